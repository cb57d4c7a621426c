"""The voice-clone encoder kernels' kernel-level entries at the boundary, on a
CPU box: the library exports and the header declares them, the ctypes
signatures load, qtts.py has the wrappers, every refusal comes back before any
device is touched, and qtts_hip_econv_plan reports the rows / kz of every case
of enc_kernel_cases.py."""
import ctypes as C
import os
import re

import pytest

import enc_kernel_cases as CS
import enc_kernel_ref as E
import qtts

NEW = ["qtts_hip_econv_plan", "qtts_hip_econv_case", "qtts_hip_enc_op", "qtts_hip_enc_func"]
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def test_library_exports_and_header_declares_the_symbols():
    lib = qtts.lib()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing
    assert set(NEW) <= set(qtts.EXPORTS)
    txt = re.sub(r"\s+", " ", open(os.path.join(INCLUDE, "qtts_hip.h")).read())
    assert "int qtts_hip_econv_plan(const qtts_econv_desc_t *d, qtts_econv_plan_t *plan_out);" in txt
    assert "int qtts_hip_econv_case(const qtts_econv_desc_t *d, qtts_econv_plan_t *plan_out, void *stream);" in txt
    assert "int qtts_hip_enc_op(const qtts_enc_op_t *d, void *stream);" in txt
    assert "int qtts_hip_enc_func(float *out_dev, const float *x_dev, size_t n, int fn, void *stream);" in txt
    # the descriptor's fields, in the header's order, are the ctypes structure's
    body = re.search(r"typedef struct \{([^}]*)\} qtts_econv_desc_t;", txt).group(1)
    names = re.findall(r"[\s*](\w+)(?:\[16\])?\s*[,;]", body)
    assert names == [f[0] for f in qtts.EConvDesc._fields_], names
    body = re.search(r"typedef struct \{([^}]*)\} qtts_econv_plan_t;", txt).group(1)
    assert re.findall(r"[\s*](\w+)\s*[,;]", body) == [f[0] for f in qtts.EConvPlan._fields_]


def test_ctypes_signatures_and_wrappers():
    lib = qtts.lib()
    vp = C.c_void_p
    want = {"qtts_hip_econv_plan": [C.POINTER(qtts.EConvDesc), C.POINTER(qtts.EConvPlan)],
            "qtts_hip_econv_case": [C.POINTER(qtts.EConvDesc), C.POINTER(qtts.EConvPlan), vp],
            "qtts_hip_enc_op": [C.POINTER(qtts.EncOp), vp],
            "qtts_hip_enc_func": [vp, vp, C.c_size_t, C.c_int, vp]}
    for name, args in want.items():
        f = getattr(lib, name)
        assert f.restype is C.c_int and list(f.argtypes) == args, name
    for w in ("econv_plan", "econv_case", "enc_op", "enc_func"):
        assert callable(getattr(qtts.Kernels, w))


@pytest.mark.parametrize("cv", CS.CASES, ids=[cv.id() for cv in CS.CASES])
def test_plan_reports_the_case(cv):
    desc, lo = CS.host_desc(cv)
    p = qtts.Kernels.econv_plan(desc)
    assert (p["rows"], p["kz"]) == (cv.rows, cv.kz) == E.plan_model(cv, lo)
    assert p["grid"] == [(cv.nmax + 63) // 64, (cv.M + 63) // 64, cv.nb * cv.kz]
    assert p["part_elems"] == (cv.kz * cv.nb * cv.M * cv.nmax if cv.kz > 1 else 0)
    if cv.name in CS.TABLE:
        assert (p["rows"], p["kz"]) == CS.TABLE[cv.name]


def test_plan_looks_at_the_input_alignment():
    desc, _ = CS.host_desc(CS.ROWS[0])
    assert qtts.Kernels.econv_plan(desc)["rows"] == 1
    desc.x += 4
    assert qtts.Kernels.econv_plan(desc)["rows"] == 0


def test_econv_refusals_without_a_device(capfd):
    """plan and case refuse the same descriptors, before any device call: the
    dummy addresses are never dereferenced (and a CPU box has no device)"""
    lib = qtts.lib()

    def plan(mutate, cv=CS.TDNN):
        desc, _ = CS.host_desc(cv)
        mutate(desc)
        return lib.qtts_hip_econv_plan(C.byref(desc), C.byref(qtts.EConvPlan()))

    def case(mutate, cv=CS.TDNN):      # only ever called with a descriptor the entry must refuse
        desc, _ = CS.host_desc(cv)
        mutate(desc)
        return lib.qtts_hip_econv_case(C.byref(desc), C.byref(qtts.EConvPlan()), None)

    def both(mutate, cv=CS.TDNN):
        return plan(mutate, cv), case(mutate, cv)

    def setf(**kw):
        def f(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return f

    def seta(name, i, v):
        def f(d):
            getattr(d, name)[i] = v
        return f
    assert plan(lambda d: None) == 0
    for m in (setf(nb=0), setf(nb=17), setf(nb=-1), setf(M=0), setf(ci=0), setf(kw=0), setf(nmax=0),
              seta("lout", 1, CS.TDNN.nmax + 1), seta("lout", 0, -1),
              seta("lin", 2, 2),        # reflect: padl 2 >= lin 2
              seta("lin", 2, 1)):
        assert both(m) == (-1, -1)
    assert both(seta("lin", 2, 384), CS.STFT) == (-1, -1)        # one below the shortest reflect accepts
    assert plan(setf(padl=1, kw=3)) == 0
    assert both(lambda d: (setattr(d, "padl", 0), d.lin.__setitem__(2, 1))) == (-1, -1)   # reflect needs lin >= 2
    # case only: operands it needs, modes it knows, a workspace that is too small
    for m in (setf(w=None), setf(x=None), setf(y=None), setf(stride=0), setf(dil=0), setf(padl=-1), setf(pmode=3)):
        assert case(m) == -1
    assert both(setf(part=1 << 20, part_elems=10), CS.STFT) == (0, -1)
    assert lib.qtts_hip_econv_plan(None, None) == -1 and lib.qtts_hip_econv_case(None, None, None) == -1
    capfd.readouterr()


def test_enc_op_and_func_refusals_without_a_device():
    lib = qtts.lib()
    P = 1 << 20

    def op(code, n_in, n_out, n, s=(1, 1, 1), drop_in=None, drop_out=None):
        d = qtts.EncOp()
        d.op = code
        for i in range(n_in):
            d.inp[i] = None if drop_in == i else P
        for i in range(n_out):
            d.out[i] = None if drop_out == i else P
        for i, v in enumerate(n):
            d.n[i] = v
        for i, v in enumerate(s):
            d.s[i] = v
        return lib.qtts_hip_enc_op(C.byref(d), None)
    assert lib.qtts_hip_enc_op(None, None) == -1
    assert op(-1, 0, 0, ()) == -1 and op(10, 0, 0, ()) == -1
    shapes = {qtts.EO_MEL: (5, 1, (513, 3, 2, 128)), qtts.EO_ROW_MEAN: (2, 1, (8, 5, 2)),
              qtts.EO_EGEMV: (2, 1, (5, 100, 100, 0, 5, 2)), qtts.EO_SE_APPLY: (4, 1, (5, 8, 2)),
              qtts.EO_ASP_STATS: (2, 1, (8, 5, 2)), qtts.EO_ASP_POOL: (3, 1, (8, 5, 2)),
              qtts.EO_LN_ROWS: (3, 1, (5, 64)), qtts.EO_ROPE_BT: (2, 1, (15, 64, 4, 16, 5)),
              qtts.EO_ROWS_BT: (0, 2, (15, 5)), qtts.EO_RVQ_ENC: (4, 1, (5, 64, 5, 100, 32, 16, 1, 5))}
    for code, (n_in, n_out, n) in shapes.items():
        for i in range(n_in):
            if not (code == qtts.EO_EGEMV and i == 2):
                assert op(code, n_in, n_out, n, drop_in=i) == -1, (code, i)
        for i in range(n_out):
            assert op(code, n_in, n_out, n, drop_out=i) == -1, (code, i)
        for i in range(len(n)):
            if not (code == qtts.EO_EGEMV and i == 3):
                assert op(code, n_in, n_out, n[:i] + (0,) + n[i + 1:]) == -1, (code, i)
    assert op(qtts.EO_MEL, 5, 1, (1041, 3, 2, 128)) == -1                     # k_mel keeps mag[1040]
    assert op(qtts.EO_EGEMV, 3, 1, (5, 100, 100, 5, 5, 2)) == -1              # unknown activation
    assert op(qtts.EO_ROPE_BT, 2, 1, (15, 64, 4, 15, 5)) == -1                # odd head_dim
    assert op(qtts.EO_ROPE_BT, 2, 1, (15, 63, 4, 16, 5)) == -1                # rows shorter than the heads
    for n in ((5, 60, 5, 100, 32, 16, 1, 5), (5, 64, 5, 100, 24, 16, 1, 5), (5, 64, 5, 100, 32, 17, 1, 5),
              (5, 64, 5, 100, 32, 16, 17, 5), (5, 64, 5, 100, 32, 16, 1, 4), (5, 64, 7, 100, 32, 16, 1, 5),
              (5, 8192, 5, 100, 32, 16, 1, 5)):
        assert op(qtts.EO_RVQ_ENC, 4, 1, n) == -1, n
    f = lib.qtts_hip_enc_func
    assert f(None, P, 4, 0, None) == -1 and f(P, None, 4, 0, None) == -1
    assert f(P, P, 0, 0, None) == -1 and f(P, P, 4, 2, None) == -1 and f(P, P, 4, -1, None) == -1
