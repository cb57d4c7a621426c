"""qtts_hip_codec_op at the boundary, on a CPU box: the library exports and the
header declares it, the ctypes structure agrees with the header field by
field, qtts.py has the wrapper, and every op refuses before any device call a
NULL descriptor, an unknown op, each operand it needs as NULL in turn, sizes
below 1 and sizes over the launch helpers' limits."""
import ctypes as C
import os
import re

import qtts

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
P = 1 << 20

# op -> (operands in, operands out, sizes that launch, index of an optional operand, sizes that may be 0)
SHAPES = {
    qtts.CO_RVQ_SUM: (2, 2, (3, 16, 12, 40), None, ()),
    qtts.CO_RVQ_PROJ: (4, 1, (40, 10, 3, 6), None, ()),
    qtts.CO_RVQ_SUM_MS: (4, 2, (18, 2, 4, 3, 16, 12, 40), None, (1,)),
    qtts.CO_RVQ_PROJ_MS: (4, 1, (40, 10, 3, 3, 6), None, ()),
    qtts.CO_DWCONV: (3, 1, (80, 6, 5, 67, 7, 70), 2, (1,)),
    qtts.CO_DWCONV_MS: (3, 1, (80, 6, 5, 67, 7, 70, 3), 2, (1,)),
    qtts.CO_LN_T: (3, 1, (70, 67, 300), None, ()),
    qtts.CO_LN_T_MS: (3, 1, (70, 67, 300, 3), None, ()),
    qtts.CO_RMS_ROWS: (2, 1, (3, 300), None, ()),
    qtts.CO_ROPE_ROWS: (2, 1, (3, 68, 4, 16), None, ()),
    qtts.CO_ROPE_KV_MS: (8, 3, (64, 4, 64, 4, 16, 4, 3, 80), None, ()),
    qtts.CO_MS_INDEX: (2, 2, (3, 5), None, ()),
    qtts.CO_CLAMP: (0, 1, (300,), None, ()),
    qtts.CO_COPY2D: (1, 1, (70, 80, 5, 67), None, ()),
    qtts.CO_CLAMP_MS: (2, 1, (300, 75, 3), None, ()),
    qtts.CO_HIST_MS: (2, 2, (80, 5, 6, 2, 3, 1), None, (5,)),
    qtts.CO_KV_SHIFT_MS: (3, 1, (6, 80, 64, 72, 5, 4), None, ()),
    qtts.CO_HIST_RESET_MS: (2, 0, (3, 11, 0), None, (1, 2)),
    qtts.CO_MS_STATE_SAVE: (3, 1, (3, 2, 11, 1, 10, 12), None, (0, 1, 2, 3, 4, 5)),
    qtts.CO_MS_STATE_LOAD: (4, 0, (3, 2, 11, 1, 10, 12), None, (0, 1, 2, 3, 4, 5)),
}
# sizes over the limits, per op: every one refused
OVER = {
    qtts.CO_RVQ_SUM: [(3, 16, 12, 1025)],
    qtts.CO_RVQ_SUM_MS: [(18, 2, 4, 3, 16, 12, 1025), (15, 2, 4, 3, 16, 12, 40)],      # vq; ldc < Q
    qtts.CO_RVQ_PROJ: [(40, 10, 3, 2), (40, 1 << 30, 3, 6)],                            # ldo < T; the grid
    qtts.CO_RVQ_PROJ_MS: [(40, 10, 3, 3, 2)],
    qtts.CO_DWCONV: [(60, 6, 5, 67, 7, 70), (80, 6, 5, 67, 7, 60)],                     # ldx < L; ldy < L
    qtts.CO_DWCONV_MS: [(60, 6, 5, 67, 7, 70, 3)],
    qtts.CO_LN_T: [(60, 67, 300)],
    qtts.CO_LN_T_MS: [(60, 67, 300, 3)],
    qtts.CO_ROPE_ROWS: [(3, 68, 4, 15), (3, 60, 4, 16)],                                # odd hd; rows shorter than the heads
    qtts.CO_ROPE_KV_MS: [(64, 4, 64, 4, 15, 4, 3, 80), (60, 4, 64, 4, 16, 4, 3, 80), (64, 4, 60, 4, 16, 4, 3, 80)],
    qtts.CO_COPY2D: [(60, 80, 5, 67), (70, 60, 5, 67)],
    qtts.CO_HIST_MS: [(4, 5, 6, 2, 3, 1)],                                              # ldx < H
    qtts.CO_KV_SHIFT_MS: [(6, 80, 64, 81, 5, 4), (6, 80, 64, 72, 70000, 4), (6, 80, 64, 72, 5, 70000)],
    qtts.CO_HIST_RESET_MS: [(70000, 11, 0)],
    qtts.CO_MS_STATE_SAVE: [(0, 0, 11, 1, 0, 0), (3, 2, 11, 1, 10, 8), (3, 2, 11, 1, 10, 13)],   # no part; kvpad < kvn; kvpad % 4
    qtts.CO_MS_STATE_LOAD: [(0, 0, 11, 1, 0, 0), (3, 2, 11, 1, 10, 10)],
}


def _op(code, n_in, n_out, n, drop_in=None, drop_out=None):
    d = qtts.CodecOp()
    d.op = code
    for i in range(n_in):
        d.inp[i] = None if drop_in == i else P
    for i in range(n_out):
        d.out[i] = None if drop_out == i else P
    for i, v in enumerate(n):
        d.n[i] = v
    d.s[0] = d.s[1] = 1 << 12
    d.eps = 1e-6
    return qtts.lib().qtts_hip_codec_op(C.byref(d), None)


def test_symbol_header_and_struct():
    lib = qtts.lib()
    assert hasattr(lib, "qtts_hip_codec_op") and "qtts_hip_codec_op" in qtts.EXPORTS
    f = lib.qtts_hip_codec_op
    assert f.restype is C.c_int and list(f.argtypes) == [C.POINTER(qtts.CodecOp), C.c_void_p]
    assert callable(qtts.Kernels.codec_op)
    txt = re.sub(r"\s+", " ", open(os.path.join(INCLUDE, "qtts_hip.h")).read())
    assert "int qtts_hip_codec_op(const qtts_codec_op_t *d, void *stream);" in txt
    body = re.search(r"typedef struct \{([^}]*)\} qtts_codec_op_t;", txt).group(1)
    fields = re.findall(r"(const void \*|void \*|int |size_t |float )(\w+)(?:\[(\d+)\])?;", body)
    ctype = {"const void *": C.c_void_p, "void *": C.c_void_p, "int ": C.c_int, "size_t ": C.c_size_t,
             "float ": C.c_float}
    want = [("inp" if name == "in" else name, ctype[t] * int(cnt) if cnt else ctype[t]) for t, name, cnt in fields]
    assert [w[0] for w in want] == [f[0] for f in qtts.CodecOp._fields_]

    class Header(C.Structure):
        _fields_ = want
    assert C.sizeof(Header) == C.sizeof(qtts.CodecOp)
    for name, _ in want:
        assert getattr(Header, name).offset == getattr(qtts.CodecOp, name).offset, name
        assert getattr(Header, name).size == getattr(qtts.CodecOp, name).size, name
    # the enum, in the header's order, is qtts.py's constants
    enum = re.search(r"enum \{ (QTTS_CO_RVQ_SUM = 0[^}]*)\}", txt).group(1)
    names = [e.strip().split(" ")[0] for e in enum.split(",")]
    assert names[-1] == "QTTS_CO_COUNT" and len(names) - 1 == len(SHAPES)
    for i, nm in enumerate(names[:-1]):
        assert getattr(qtts, nm[len("QTTS_"):]) == i, nm
    # the header's table lists every op by its kernel
    import codec_op_cases as CS
    for i, k in enumerate(sorted(CS.KERNELS)):
        assert re.search(rf"\b\d+ {k}\b", txt), k


def test_refusals_without_a_device():
    """every refusal comes back before any device call: the dummy addresses are
    never dereferenced (and a CPU box has no device)"""
    lib = qtts.lib()
    assert lib.qtts_hip_codec_op(None, None) == -1
    assert _op(-1, 0, 0, ()) == -1 and _op(len(SHAPES), 0, 0, ()) == -1
    for code, (n_in, n_out, n, opt, zero_ok) in SHAPES.items():
        for i in range(n_in):
            if i != opt:
                assert _op(code, n_in, n_out, n, drop_in=i) == -1, (code, "in", i)
        for i in range(n_out):
            assert _op(code, n_in, n_out, n, drop_out=i) == -1, (code, "out", i)
        for i in range(len(n)):
            bad = -1 if i in zero_ok else 0
            assert _op(code, n_in, n_out, n[:i] + (bad,) + n[i + 1:]) == -1, (code, "n", i)
        for over in OVER.get(code, ()):
            assert _op(code, n_in, n_out, over) == -1, (code, over)
