"""The nucleus short-list sampler's kernel-level entries at the boundary, on a
CPU box: the library exports and the header declares them, the ctypes
signatures load, qtts.py has the wrappers, and both refuse bad arguments
before any device is touched."""
import ctypes as C
import math
import os
import re

import qtts

NEW = ["qtts_hip_sample_nucleus", "qtts_hip_sample_nucleus_rows"]
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def test_library_exports_and_header_declares_the_symbols():
    lib = qtts.lib()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing
    assert set(NEW) <= set(qtts.EXPORTS)
    txt = re.sub(r"\s+", " ", open(os.path.join(INCLUDE, "qtts_hip.h")).read())
    assert ("int qtts_hip_sample_nucleus(int *out_dev, const float *logits_dev, int vocab, int top_k, float top_p, "
            "float temperature, uint32_t *rng_bits_dev, int batch, void *stream, int *path_dev);") in txt
    assert ("int qtts_hip_sample_nucleus_rows(int *out_dev, int *path_dev, const float *logits_dev, int vocab, "
            "const int *top_k, const float *top_p, const float *temperature, uint32_t *rng_bits_dev, int batch, "
            "int eos, int redraw, void *stream);") in txt


def test_ctypes_signatures_and_wrappers():
    lib = qtts.lib()
    ip, fp, vp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_void_p
    want = {"qtts_hip_sample_nucleus": [vp, vp, C.c_int, C.c_int, C.c_float, C.c_float, vp, C.c_int, vp, vp],
            "qtts_hip_sample_nucleus_rows": [vp, vp, vp, C.c_int, ip, fp, fp, vp, C.c_int, C.c_int, C.c_int, vp]}
    for name, args in want.items():
        f = getattr(lib, name)
        assert f.restype is C.c_int and list(f.argtypes) == args, name
    assert callable(qtts.Kernels.sample_nucleus) and callable(qtts.Kernels.sample_nucleus_rows)


def test_entries_refuse_bad_arguments_without_a_device():
    """every refusal comes before the first device call: the dummy pointers
    below are never dereferenced (and a CPU box has no device to touch)"""
    lib = qtts.lib()
    p = C.c_void_p(64)   # a non-NULL dummy
    k, f, t = (C.c_int * 2)(50, 0), (C.c_float * 2)(0.8, 0.9), (C.c_float * 2)(0.9, 1.1)

    def plain(out=p, logits=p, vocab=2048, top_k=50, top_p=0.8, temp=0.9, rng=p, batch=2):
        return lib.qtts_hip_sample_nucleus(out, logits, vocab, top_k, top_p, temp, rng, batch, None, None)

    def rows(out=p, logits=p, vocab=2048, top_k=k, top_p=f, temp=t, rng=p, batch=2, eos=-1, redraw=0):
        return lib.qtts_hip_sample_nucleus_rows(out, None, logits, vocab, top_k, top_p, temp, rng, batch, eos,
                                                redraw, None)
    for fn in (plain, rows):
        assert fn(out=None) == -1 and fn(logits=None) == -1 and fn(rng=None) == -1
        assert fn(batch=0) == -1 and fn(batch=-3) == -1
        assert fn(vocab=0) == -1 and fn(vocab=4097) == -1
    assert rows(top_k=None) == -1 and rows(top_p=None) == -1 and rows(temp=None) == -1
    for bad in (0.0, -0.5, math.nan, math.inf, -math.inf):
        assert plain(top_p=bad) == -1, bad
        assert rows(top_p=(C.c_float * 2)(0.8, bad)) == -1, bad
    for bad in (math.nan, math.inf, -math.inf):
        assert plain(temp=bad) == -1, bad
        assert rows(temp=(C.c_float * 2)(bad, 0.9)) == -1, bad
    assert rows(eos=2048, redraw=1) == -1   # the EOS id lies outside the vocabulary
