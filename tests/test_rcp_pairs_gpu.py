"""The paired reciprocal of the one-round free-body step's row constants
(test_isaacgym_amd/csrc/mg_pair.h rcp2_ieee, run over a device array by
mg_debug_rcp_pairs) against IEEE division: numpy's np.float32(1) / d, compared
by bit pattern, a NaN against a NaN. One launch over 34,553 values:

  - +-0, +-inf and a quiet NaN;
  - the smallest and the largest denormal, both signs;
  - every exponent 1..254 with the mantissas 0, 1, 0x400000, 0x7fffff and 64
    seeded random ones, both signs: the exponents at which v_div_scale scales
    the denominator or the numerator, and the quotients that are denormal, are
    among them;
  - an odd element count, so the last pair is half empty.
"""
import numpy as np
import pytest
import torch

from test_isaacgym_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 61


def _inputs():
    rng = np.random.default_rng(SEED)
    exps = np.arange(1, 255, dtype=np.uint32)
    fixed = np.broadcast_to(np.array([0, 1, 0x400000, 0x7FFFFF], np.uint32), (2, 254, 4))
    rand = rng.integers(0, 1 << 23, (2, 254, 64), dtype=np.uint32)   # fresh ones per exponent and sign
    mant = np.concatenate([fixed, rand], axis=2)
    sign = np.array([0, 0x80000000], np.uint32)[:, None, None]
    normal = (sign | (exps[None, :, None] << 23) | mant).ravel()
    special = np.array([0x00000000, 0x7F800000, 0x00000001, 0x007FFFFF], np.uint32)
    bits = np.concatenate([special, special | np.uint32(0x80000000), np.array([0x7FC00000], np.uint32), normal])
    if len(bits) % 2 == 0:
        bits = np.concatenate([bits, np.array([0x40400000], np.uint32)])   # 3.0: an odd count
    return bits.view(np.float32)


def test_rcp_pairs_equal_ieee_division_bits():
    d = _inputs()
    assert len(d) % 2 == 1 and len(d) >= 2 * 254 * 68 + 9
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        want = (np.float32(1) / d).astype(np.float32)
    dd = torch.from_numpy(d.copy()).to(DEV)
    out = torch.full((len(d) + 1,), 7.0, dtype=torch.float32, device=DEV)   # one past the end: a guard
    torch.cuda.synchronize()
    N.check(N.lib.mg_debug_rcp_pairs(dd.data_ptr(), out.data_ptr(), len(d)), "mg_debug_rcp_pairs")
    got = out.cpu().numpy()
    assert got[-1] == 7.0, "the half-empty last pair wrote past the end"
    got = got[:-1]
    nan_w, nan_g = np.isnan(want), np.isnan(got)
    assert np.array_equal(nan_w, nan_g), "NaN where IEEE has none (or the reverse): %s" % d[nan_w != nan_g][:8]
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan_w
    assert not bad.any(), "%d of %d differ, e.g. d = %s: got %s, IEEE %s" % (
        bad.sum(), len(d), d[bad][:4].view(np.uint32), got[bad][:4].view(np.uint32), want[bad][:4].view(np.uint32))
    assert N.lib.mg_debug_rcp_pairs(None, None, 4) < 0 and N.lib.mg_debug_rcp_pairs(None, None, 0) == 0
