"""The HIP sources have one build variant besides the release: the diagnostic
build (-DAMH_STAMPS / -DAMH_DIAG, `make stamps`).  Concluded A/B experiments
leave as rows of DESIGN.md's "Retired experiments" table, not as compile
switches, so every preprocessor conditional under csrc/ names only those two
macros (CPU)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adaptive-mcmc_amd", "csrc")
ALLOWED = {"AMH_STAMPS", "AMH_DIAG"}
CONDITIONAL = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$")


def test_conditionals_name_only_the_diagnostic_build():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert files
    bad, seen = [], 0
    for path in files:
        for no, line in enumerate(open(path), 1):
            m = CONDITIONAL.match(line)
            if m is None:
                continue
            seen += 1
            cond = m.group(2).split("//")[0]
            names = set(re.findall(r"[A-Za-z_]\w*", cond)) - {"defined"}
            if not names or not names <= ALLOWED:
                bad.append(f"{os.path.basename(path)}:{no}: {line.strip()}")
    assert seen > 0  # the diagnostic build's own conditionals were found
    assert not bad, "compile switches other than AMH_STAMPS / AMH_DIAG:\n" + "\n".join(bad)
