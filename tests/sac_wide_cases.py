"""Shared pieces of the wide-batch SAC tests (tests/test_sac_wide_cpu.py, tests/test_sac_wide_gpu.py): the pinned shapes and seeds of
the update-parity cases above 512 rows and the check of a reference pair (the torch step in float32 against float64).

At large batches the torch step alone does not meet the learner tolerances (sac_cases.TOL) on every input: one step can take the
other side of a ReLU mask, of min(Q1, Q2) or of the log_std clamp in the two precisions, and a handful of Adam moments then differ
by several bounds.  The shapes below are the ones on which the pair agrees with margin on the CPU (worst |diff| / bound 0.0073 to
0.111 over both seeds, after 1 and 3 steps), so a parity test on them tells a kernel bug from an input that no float32 step could pass.
If a pair fails, its seed is replaced by the next integer that passes and the change is recorded here; the tolerance is never touched.

Replaced so far.  The GPU test draws its noise from fw_sac_noise (Philox), not sac_cases.make_noise, so its inputs are not the CPU
test's.  On an MI355X (worst |diff| / bound of the float32 / float64 pair after 1 and 3 steps, seeds 5 to 9 of every shape):
(21, 6, 256, 1024) leaves the tolerances with seed 5 (2.75 x after 3 steps), 6 (1.44 x) and 7 (6.86 x) and passes with 8 (0.40) and
9 (0.03): on the GPU its seeds are 8 and 9.  Every other shape passes with seeds 5 and 6 (worst 0.78, (21, 6, 64, 8192) seed 5).
The CPU test runs the replacement seeds too."""
import pytest

from pyflyt_drone_amd import sac as S

import sac_cases as SC

# (obs_dim, act_dim, hidden, batch): 576 is the smallest wide batch (a ragged last 512-row split, a ragged last 256-row workgroup),
# 1024 at H 256 two full splits, 8192 at H 64 all 16 splits and all 64 partial-sum slots of the head stage
WIDE_SHAPES = [(21, 6, 64, 576), (21, 6, 256, 1024), (28, 4, 256, 2048), (30, 3, 64, 4096), (21, 6, 64, 8192)]
# seeds per shape: sac_cases.SEEDS unless a pair had to be replaced (above)
WIDE_SEEDS_GPU = {shape: list(SC.SEEDS) for shape in WIDE_SHAPES}
WIDE_SEEDS_GPU[(21, 6, 256, 1024)] = [8, 9]
WIDE_CASES_GPU = [shape + (seed,) for shape in WIDE_SHAPES for seed in WIDE_SEEDS_GPU[shape]]
WIDE_CASES_CPU = [shape + (seed,) for shape in WIDE_SHAPES for seed in sorted(set(SC.SEEDS) | set(WIDE_SEEDS_GPU[shape]))]

SCALAR_TOL = dict(rel=2e-3, abs=1e-5)


def compare_scalars(sa, sb, what):
    for k in S.SCALARS:
        assert float(sa[k]) == pytest.approx(float(sb[k]), **SCALAR_TOL), (what, k, float(sa[k]), float(sb[k]))


def check_reference_pair(p32, o32, s32, p64, o64, s64, case, step):
    """torch float32 against torch float64 under the learner tolerances: a failure means the pinned input is invalid, not the kernel."""
    try:
        SC.compare(p32, o32, p64, o64)
        compare_scalars(s32, s64, "reference pair")
    except AssertionError as e:
        pytest.fail(f"the pinned input {case} is invalid: the torch step in float32 leaves the learner tolerances against float64 after "
                    f"{step + 1} step(s) ({e}); pick the next seed in tests/sac_wide_cases.py")
