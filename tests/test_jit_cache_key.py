"""The compile options of a specialised program are part of its cache key (csrc/gmx_kernels.hip, jit_cache_path): the same
translation unit under two option strings is kept in two files, so a code object built with other options is never loaded
in place of this build's.  Host code only: no compile, no GPU."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "genjax_amd", "lib", "libgenmi_hip.so"))
    lib.gmx_jit_cache_path_of.restype = ctypes.c_size_t
    lib.gmx_jit_cache_path_of.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    lib.gmx_jit_options_of.restype = ctypes.c_size_t
    lib.gmx_jit_options_of.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    return lib


def _path(lib, src, opts):
    buf = ctypes.create_string_buffer(4096)
    n = lib.gmx_jit_cache_path_of(src.encode(), opts.encode(), buf, len(buf))
    assert n == len(buf.value)
    return buf.value.decode()


def _options(lib, flags):
    buf = ctypes.create_string_buffer(512)
    assert lib.gmx_jit_options_of(flags, buf, len(buf)) == len(buf.value)
    return buf.value.decode()


def test_options_enter_the_cache_key(tmp_path, monkeypatch):
    monkeypatch.setenv("GENMI_JIT_CACHE", str(tmp_path))
    lib = _lib()
    src = '#include "gmx_jit.h"\nGMX_JIT_BEGIN(16, false, 0, 4, 0)\nGMX_JIT_END\n'
    a = _path(lib, src, "--offload-arch=gfx950 -O3 ")
    b = _path(lib, src, "--offload-arch=gfx950 -O3 -fno-slp-vectorize ")
    assert a.startswith(str(tmp_path) + "/") and b.startswith(str(tmp_path) + "/") and a.endswith(".co")
    assert a != b
    assert a == _path(lib, src, "--offload-arch=gfx950 -O3 ")              # a key, not a counter
    assert a != _path(lib, src + " ", "--offload-arch=gfx950 -O3 ")        # the source is still in it
    monkeypatch.setenv("GENMI_JIT_CACHE", "0")
    assert _path(lib, src, "--offload-arch=gfx950 -O3 ") == ""


def test_program_kinds_have_their_own_options(tmp_path, monkeypatch):
    """a chain program (plain, resample-first, looped, sharded) is compiled without the SLP vectoriser, a background
    program with it: two option strings, hence two cache files even for the same source"""
    monkeypatch.setenv("GENMI_JIT_CACHE", str(tmp_path))
    lib = _lib()
    chain, background = _options(lib, 0), _options(lib, 2)
    for flags in (1, 4, 8):
        assert _options(lib, flags) == chain
    assert "-fno-slp-vectorize" in chain.split() and "-fno-slp-vectorize" not in background.split()
    for o in (chain, background):
        assert {"--offload-arch=gfx950", "-O3", "-ffp-contract=off"} <= set(o.split())
    assert _path(lib, "x", chain) != _path(lib, "x", background)
