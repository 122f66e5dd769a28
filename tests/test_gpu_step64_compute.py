"""The d = 64 step kernel's compute phase (arwmh_step64_kernel, ARWMH and
ASSS): in a single-step ARWMH launch the proposal's and the potential's
broadcast vectors travel through scalar registers (v_readlane in batches, no
LDS scratch), in a fused launch and in ASSS through the wave's scratch, and
the swap reads its columns unmasked.  The schedule's gamma_n is pinned along
with them -- the reset of n at i == W inside a fused launch and on a launch's
first step, and the end of the gamma table inside a launch -- so that a
kernel that fetches gamma ahead of its step (tried and measured without gain,
DESIGN.md 5) has its cases waiting.

Every comparison is bit for bit against the C oracle on whole states (states
that hold NaN: identical NaN positions, every other word identical -- the
payload of a default NaN differs between the two machines).  The helpers are
those of test_gpu_step64_swap: a factor whose 2,080 packed entries all differ
and, but for the launch that has to straddle the reset, num_warmup = 2.

Shapes: C = 1 (one wave works, fifteen never enter the loop), C = 17 (two
blocks, one wave with two items), C = 4,097 = 256 * 16 + 1 (every CU has one
item per wave and one wave has two)."""
import numpy as np
import pytest
import torch

from helpers import ASSS_FIELDS, _leaf, assert_state_bitequal, assert_state_bitequal_nan
from test_gpu_step64_order import _start
from test_gpu_step64_swap import _col, _distinct_factor, _set_scale

pytestmark = pytest.mark.gpu

W = 2
SHAPES = [1, 17, 4097]
GAMMA_TAB = 1 << 20  # amh_internal.h kGammaTab: gamma_n comes from the table for n < 2^20


def _start_distinct(C, orc, cls="ARWMH", num_warmup=W):
    """test_gpu_step64_swap._start_distinct at any num_warmup"""
    k, st, om, ost = _start(C, orc, num_warmup, cls=cls)
    L = _distinct_factor(C)
    _set_scale(st, L)
    _set_scale(ost, L)
    torch.cuda.synchronize()
    return k, st, om, ost


def _set_i(st, ost, i0):
    st.i.fill_(i0)
    ost.i[...] = i0
    torch.cuda.synchronize()


@pytest.mark.parametrize("num_warmup", [2, 6])
@pytest.mark.parametrize("C", SHAPES)
def test_arwmh_single_then_fused(C, num_warmup, gpu, orc):
    """Four single-step launches (i = 0 .. 3), then one fused launch of five
    steps (i = 4 .. 8).  num_warmup = 6: the fused launch straddles i == W, the
    reset of n falls inside it (gamma_1 = 1: that step keeps L).  num_warmup =
    2, the swap tests' setting: the reset falls on the first step of the third
    single launch."""
    k, st, om, ost = _start_distinct(C, orc, num_warmup=num_warmup)
    for t in range(4):
        k.sample_(st, 1)
        orc.step(om, ost, 1, num_warmup=num_warmup)
        torch.cuda.synchronize()
        assert_state_bitequal(st, ost, f"C={C} W={num_warmup} launch {t + 1}")
    k.sample_(st, 5)
    orc.step(om, ost, 5, num_warmup=num_warmup)
    torch.cuda.synchronize()
    assert_state_bitequal(st, ost, f"C={C} W={num_warmup} fused launch of five")
    assert int(ost.i[0]) == 9


@pytest.mark.parametrize("cls", ["ARWMH", "ASSS"])
def test_gamma_table_end_inside_a_launch(cls, gpu, orc):
    """A fused launch of five steps started two steps below the end of the
    gamma table: n = 2^20 - 2, 2^20 - 1 come from the table, n = 2^20 ..
    2^20 + 2 from lr_gamma_slow."""
    C = 17
    k, st, om, ost = _start_distinct(C, orc, cls=cls)
    i0 = GAMMA_TAB - 2 + W - 1  # n = i + 1 - W
    _set_i(st, ost, i0)
    k.sample_(st, 5)
    if cls == "ARWMH":
        orc.step(om, ost, 5, num_warmup=W)
    else:
        orc.asss_step(om, ost, 5, num_warmup=W)
    torch.cuda.synchronize()
    assert int(ost.i[0]) == i0 + 5 and i0 + 1 - W < GAMMA_TAB <= i0 + 5 - W
    if cls == "ARWMH":
        assert_state_bitequal(st, ost, "gamma table end, ARWMH")
    else:
        from test_gpu_asss import assert_bitequal
        assert_bitequal(st, ost, "gamma table end, ASSS")


# bit patterns the broadcasts have to carry, by either route (helpers.EDGE_VALUES)
PATTERNS = (np.nan, np.inf, -np.inf, -0.0, 1e-45)


def _inject(state, C):
    """Chain 2 p + 1 holds pattern p in z (coordinates 0, 31, 63), chain 2 p + 2
    in loc; chain 12 has L_31,31 = 0 (eta_31 = 0 * xi: a signed zero in the
    proposal's vector, and a reverted update)."""
    z, loc, scale = (_leaf(state, f) for f in ("z", "loc", "scale"))
    host = [a.detach().cpu().numpy().copy() if torch.is_tensor(a) else a for a in (z, loc, scale)]
    for p, v in enumerate(PATTERNS):
        host[0][2 * p + 1, [0, 31, 63]] = np.float32(v)
        host[1][2 * p + 2, [0, 31, 63]] = np.float32(v)
    host[2][12, _col(31)] = 0.0
    assert C > 12
    for a, h in zip((z, loc, scale), host):
        if torch.is_tensor(a):
            a.copy_(torch.from_numpy(h))


@pytest.mark.parametrize("cls", ["ARWMH", "ASSS"])
def test_every_bit_pattern_is_carried(cls, gpu, orc):
    """z or loc with NaN, +-inf, -0.0 and a denormal, and a zero diagonal entry:
    three single launches and a fused one of three."""
    C = 17
    k, st, om, ost = _start_distinct(C, orc, cls=cls)
    _inject(st, C)
    _inject(ost, C)
    torch.cuda.synchronize()
    assert np.signbit(ost.z[7, 31]) and ost.z[7, 31] == 0.0 and 0.0 < ost.z[9, 0] < 1e-38
    ostep = orc.step if cls == "ARWMH" else orc.asss_step
    fields = () if cls == "ARWMH" else (ASSS_FIELDS,)
    for t, n in enumerate([1, 1, 1, 3]):
        k.sample_(st, n)
        ostep(om, ost, n, num_warmup=W)
        torch.cuda.synchronize()
        assert_state_bitequal_nan(st, ost, f"{cls} bit patterns, launch {t + 1}", *fields)
    # the finite chains are untouched by their neighbours: no NaN anywhere in them
    clean = np.setdiff1d(np.arange(C), np.arange(1, 13))
    assert np.isfinite(ost.z[clean]).all() and np.isfinite(ost.scale[clean]).all()


@pytest.mark.parametrize("C", SHAPES)
def test_asss_single_then_fused(C, gpu, orc):
    """ASSS d = 64 (S z, S v and every shrink step's potential share the
    proposal's and the potential's pieces with ARWMH): two single launches and
    one fused launch of three, against orc.asss_step."""
    from test_gpu_asss import assert_bitequal
    k, st, om, ost = _start_distinct(C, orc, cls="ASSS")
    for t, n in enumerate([1, 1, 3]):
        k.sample_(st, n)
        orc.asss_step(om, ost, n, num_warmup=W)
        torch.cuda.synchronize()
        assert_bitequal(st, ost, f"ASSS C={C} launch {t + 1} ({n} steps)")
