"""The wide form of the SAC gradient step (512 < B <= 8192) without a GPU: the batch rule in `sac.fits` and in the library, the
workspace size (unchanged up to 512 rows, larger above), and the reference pair -- sac_update_torch in float32 against float64 -- on
the pinned inputs of the GPU parity test (tests/test_sac_wide_gpu.py)."""
import pytest
import torch

from pyflyt_drone_amd import _lib
from pyflyt_drone_amd import config as K
from pyflyt_drone_amd import sac as S

import sac_cases as SC
import sac_wide_cases as WC


def test_fits_takes_the_wide_batches_and_keeps_the_rejections():
    assert (S.MAX_BATCH, S.MAX_BATCH_WIDE, S.WIDE_BATCH_MULTIPLE) == (512, 8192, 64)
    for b in (16, 512, 576, 1024, 4096, 8192):
        assert S.fits(21, 6, 256, b), b
    for b in (528, 520, 8256, 24, 0, 8, 600, 16384):
        assert not S.fits(21, 6, 256, b), b
    assert not S.fits(65, 6, 256, 1024) and not S.fits(21, 9, 256, 1024) and not S.fits(21, 6, 128, 1024)


def _workspace_floats_up_to_512(d, A, H, B):
    """The workspace of the 24-launch form, block by block (csrc/fwsim_sac.hpp: every block rounded up to four floats)."""
    blocks = [2 * B * A, 2 * B * H, 2 * B * H, 2 * B * 2 * A, 2 * B, B * (d + A), B * (d + A), 4 * B * H, 4 * B * H, 4 * B, 2 * B,
              2 * B * H, 2 * B * H, 2 * B * (d + A), B * 2 * A, 16]
    return sum((n + 3) // 4 * 4 for n in blocks)


# fw_sac_update_workspace_bytes of the build before the wide form
PARENT_WORKSPACE_BYTES = {(21, 6, 256, 512): 8724544, (21, 6, 64, 512): 2433088, (64, 8, 256, 512): 9125952, (21, 6, 256, 256): 4362304,
                          (30, 3, 64, 16): 76096}


def test_workspace_bytes_of_the_library():
    L = _lib.lib()
    for shape, want in PARENT_WORKSPACE_BYTES.items():
        assert 4 * _workspace_floats_up_to_512(*shape) == want          # (the arithmetic here is the parent build's)
        assert L.fw_sac_update_workspace_bytes(*shape) == want, shape
    for d, A, H in ((21, 6, 256), (21, 6, 64), (64, 8, 256)):
        trained = S.image_layout(d, A, H)["trained"]
        for B in (576, 1024, 8192):
            got = L.fw_sac_update_workspace_bytes(d, A, H, B)
            # the 24-launch blocks at this B, three stages x 64 partial sums, ceil(B / 512) partial gradients of every trained parameter
            want = _workspace_floats_up_to_512(d, A, H, B) + 3 * 64 + ((-(-B // 512) * trained + 3) // 4 * 4)
            assert got == 4 * want > 0, (d, A, H, B)
    assert L.fw_sac_update_workspace_bytes(64, 8, 256, 8192) // 4 < 2**31          # the kernels index it with int
    for B in (528, 8256, 520, 24):
        assert L.fw_sac_update_workspace_bytes(21, 6, 256, B) == K.FW_EUNSUPPORTED, B
        assert b"multiples of 64 in (512, 8192]" in L.fw_last_error(None)
    assert L.fw_sac_update_workspace_bytes(21, 6, 256, 0) == K.FW_EINVAL


def test_the_learner_states_the_rule():
    class Env:
        device, num_envs, obs_dim, act_dim = "cpu", 64, 21, 6

    with pytest.raises(ValueError, match=r"multiples of 64 in \(512, 8192\]"):
        S.SAC(Env(), S.SACConfig(batch_size=528, net_arch=(64, 64)))
    with pytest.raises(ValueError, match="one vec-step"):
        S.SAC(Env(), S.SACConfig(batch_size=1024, net_arch=(64, 64), buffer_size=63))


@pytest.mark.parametrize("d,A,H,B,seed", WC.WIDE_CASES_CPU)
def test_update_in_float32_matches_float64_on_the_wide_cases(d, A, H, B, seed):
    """The pinned inputs of the wide GPU parity test (the form of tests/test_sac_cpu.py::test_update_in_float32_matches_float64): no
    element of any parameter or Adam moment may leave the learner tolerances after 1 and after 3 gradient steps.  All ten cases pass
    with sac_cases.SEEDS, no seed had to be replaced here; the seeds the GPU test had to take instead (tests/sac_wide_cases.py) run too."""
    cfg = S.SACConfig(batch_size=B, net_arch=(H, H), seed=seed)
    pol = SC.make_policy(d, A, H, seed)
    rows = SC.make_batch(d, A, B, seed)
    p32, o32 = SC.learner(pol, cfg)
    p64, o64 = SC.learner(pol, cfg, dtype=torch.float64)
    for step in range(3):
        eps = SC.make_noise(A, B, seed, step)
        s32 = S.sac_update_torch(p32, o32, rows, eps[0], eps[1], cfg)
        s64 = S.sac_update_torch(p64, o64, rows.double(), eps[0].double(), eps[1].double(), cfg)
        if step in (0, 2):
            SC.compare(p32, o32, p64, o64)
            WC.compare_scalars(s32, s64, "float32 against float64")
    assert p32.n_updates == 3
