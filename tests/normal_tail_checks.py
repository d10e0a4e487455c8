"""Inputs and references shared by tests/test_normal_tail_cpu.py (the C-ABI's CPU mirror) and tests/test_normal_tail_gpu.py
(the device library): the tail of the normal draw — gmx_std_normal_from_bits (csrc/gmx_rng.h) over every input a draw can
have — and gmx_logf (csrc/gmx_math.h) around everything its exponent / mantissa split can get wrong.  The references are
the oracle's own restatements (orc_std_normal_from_bits, orc_logf), computed once per process."""
import ctypes

import numpy as np

from oracle import genjax_oracle as O

_REF = {}


def normal_bits():
    """all 2^23 distinct inputs of a draw: the tail reads bits >> 9 only"""
    return (np.arange(1 << 23, dtype=np.uint32) << np.uint32(9)).astype(np.uint32)


def normal_ref():
    if "normal" not in _REF:
        b = normal_bits()
        out = np.empty(b.size, dtype=np.float32)
        O.lib().orc_std_normal_from_bits(ctypes.c_int64(b.size), b.ctypes.data_as(ctypes.c_void_p),
                                         out.ctypes.data_as(ctypes.c_void_p))
        _REF["normal"] = out
    return _REF["normal"]


_THRESHOLD = 0x3504f3          # the mantissa of sqrt(1/2) in f32 (0x3f3504f3): where the split changes sides


def log_bits():
    """the fixed set, as bit patterns: every exponent x the 64 mantissas straddling the threshold and 0, 1, 0x7fffff; all
    mantissas at exponents 126 and 127 (x in [1/2, 2)); the first and last 4096 denormals; +-0, +-inf, negatives, NaNs"""
    mant = np.concatenate([np.arange(_THRESHOLD - 32, _THRESHOLD + 32), [0, 1, 0x7fffff]]).astype(np.uint32)
    assert mant.size == 67
    expo = np.arange(256, dtype=np.uint32)
    grid = ((expo[:, None] << np.uint32(23)) | mant[None, :]).reshape(-1)
    allm = np.arange(1 << 23, dtype=np.uint32)
    dense = np.concatenate([(np.uint32(126) << np.uint32(23)) | allm, (np.uint32(127) << np.uint32(23)) | allm])
    den = np.concatenate([np.arange(1, 4097), np.arange(0x800000 - 4096, 0x800000)]).astype(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000,                      # +-0, +-inf
                        0x80000001, 0x807fffff, 0x80800000, 0xbf800000, 0xbf3504f3, 0xff7fffff,   # negatives
                        0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0xffffffff], dtype=np.uint32)   # NaNs
    return np.concatenate([grid, dense, den, special]).astype(np.uint32)


def log_ref():
    if "log" not in _REF:
        with np.errstate(all="ignore"):
            _REF["log"] = O.log(log_bits().view(np.float32))
    return _REF["log"]


def same_or_both_nan(got, ref):
    """index of the first element that differs (None when none does): equal bits, or NaN on both sides"""
    got, ref = np.asarray(got, np.float32).reshape(-1), np.asarray(ref, np.float32).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad = (got.view(np.uint32) != ref.view(np.uint32)) & ~(np.isnan(got) & np.isnan(ref))
    return int(np.flatnonzero(bad)[0]) if bad.any() else None


def hold_normal(be, to_dev):
    """gmx_std_normal_from_bits of library `be` in ONE call over all 2^23 inputs against the oracle, bit for bit"""
    import torch
    b = normal_bits()
    bits = to_dev(torch.from_numpy(b.view(np.int32)))
    out = to_dev(torch.full((b.size,), float("nan"), dtype=torch.float32))
    be.check(be.c.gmx_std_normal_from_bits(be.ptr(bits), b.size, be.ptr(out), be.stream()), "gmx_std_normal_from_bits")
    got, ref = out.cpu().numpy(), normal_ref()
    assert not np.isnan(ref).any()
    diff = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
    assert diff.size == 0, (diff.size, [(hex(int(b[i])), float(got[i]), float(ref[i])) for i in diff[:5]])


def hold_log(to_dev):
    """the log op of the site-program VM (one traced op, one launch) over the fixed set against orc_logf"""
    import torch
    from genjax_amd import numpy as jnp
    b = log_bits()
    x = to_dev(torch.from_numpy(b.view(np.float32).copy()))
    got = jnp.log(x).cpu().numpy()
    ref = log_ref()
    assert np.isnan(ref[-5:]).all() and np.isnan(ref[-11:-5]).all() and ref[-15] == -np.inf and ref[-13] == np.inf
    i = same_or_both_nan(got, ref)
    assert i is None, (hex(int(b[i])), float(got[i]), float(ref[i]))
