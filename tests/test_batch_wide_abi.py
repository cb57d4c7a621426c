"""The 64-slot lock-step limit at the drop-in boundary, on a CPU box: both
headers define it, the library exports the wide-batch entry points and the
binding declares them, the entries refuse bad arguments without touching a
device, and the product still links nothing from oracle/."""
import ctypes as C
import os
import re
import subprocess

import qtts
from conftest import ROOT

NEW_SYMBOLS = ["qtts_hip_batch_matvec_case", "qtts_hip_gemv_wide_launches", "qtts_hip_batch_matvec_plan"]


def _define(header, name):
    txt = open(os.path.join(ROOT, "include", header)).read()
    m = re.search(rf"^#define\s+{name}\s+(\d+)\s*$", txt, re.M)
    assert m, f"{header} does not define {name}"
    return int(m.group(1))


def test_both_headers_define_the_limit_as_64():
    assert _define("qtts_hip.h", "QTTS_HIP_MAX_BATCH") == 64
    assert _define("qwen_tts.h", "QWEN_TTS_MAX_BATCH") == 64
    assert qtts.MAX_BATCH == 64


def test_library_exports_and_binding_declares_the_wide_batch_symbols():
    lib = qtts.lib()
    missing = [s for s in NEW_SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    assert set(NEW_SYMBOLS) <= set(qtts.EXPORTS)
    assert lib.qtts_hip_gemv_wide_launches.restype is C.c_longlong
    assert lib.qtts_hip_batch_matvec_case.argtypes[0] is C.POINTER(qtts.BGemvDesc)
    assert callable(qtts.Kernels.batch_matvec_case) and callable(qtts.Kernels.gemv_wide_launches)
    assert lib.qtts_hip_batch_matvec_plan.argtypes == [C.POINTER(qtts.BGemvDesc), C.POINTER(qtts.BGemvPlan)]
    assert callable(qtts.Kernels.batch_matvec_plan)
    # the descriptor and the plan mirror qtts_bgemv_desc_t / qtts_bgemv_plan_t field for field
    txt = open(os.path.join(ROOT, "include", "qtts_hip.h")).read()
    for ctype, mirror in (("qtts_bgemv_desc_t", qtts.BGemvDesc), ("qtts_bgemv_plan_t", qtts.BGemvPlan)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % ctype, txt).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            parts = [p.strip() for p in decl.split(",") if p.strip()]
            names += [re.sub(r"\[\d+\]$", "", re.sub(r"^.*[\s\*]", "", p)) for p in parts]
        assert names == [f[0] for f in mirror._fields_], names


def test_batch_matvec_case_refuses_bad_arguments_before_any_device_work():
    lib = qtts.lib()
    one = C.c_void_p(16)   # never dereferenced: the argument checks come first

    def desc(**kw):
        d = qtts.BGemvDesc()
        d.rows, d.cols, d.batch, d.A, d.x, d.ldx, d.y, d.ldy = 256, 128, 32, one, one, 128, one, 256
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert lib.qtts_hip_batch_matvec_case(None, None) == -1
    for bad in (dict(A=None), dict(x=None), dict(y=None), dict(rows=0), dict(cols=0), dict(batch=1), dict(batch=65),
                dict(epi=5), dict(epi=-1), dict(src=3), dict(src=1), dict(src=2, table=one),   # tables need ids too
                dict(epi=1), dict(epi=2),                          # bias epilogues need the bias
                dict(part_in=one, n_part_in=0), dict(part_in=one, n_part_in=5),
                dict(part_in=one, n_part_in=2, src=1, table=one, ids=one),
                dict(kz=1), dict(kz=5), dict(kz=-2),
                dict(kz=2, self_reduce=0), dict(kz=2, self_reduce=1, y=None)):
        assert lib.qtts_hip_batch_matvec_case(C.byref(desc(**bad)), None) == -1, bad
        assert lib.qtts_hip_batch_matvec_plan(C.byref(desc(**bad)), C.byref(qtts.BGemvPlan())) == -1, bad
    assert lib.qtts_hip_batch_matvec_plan(C.byref(desc()), None) == -1
    assert lib.qtts_hip_batch_matvec_plan(C.byref(desc()), C.byref(qtts.BGemvPlan())) == 0


def test_slot_limit_refused_before_the_device(capfd):
    """more than 64 slots: -1 and the limit named, from a ctx that has no device model at all"""
    lib = qtts.lib()
    ctx = qtts.Ctx()
    n = 65
    tx = (C.c_char_p * n)(*[b"1,2,3"] * n)
    out, ns = (C.c_void_p * n)(), (C.c_int * n)()
    assert lib.qwen_tts_generate_batch(C.byref(ctx), n, tx, None, None, out, ns) == -1
    assert "65 slots, at most 64" in capfd.readouterr().err
    assert all(not o for o in out)
    assert lib.qwen_tts_generate_voice_clone_batch(C.byref(ctx), n, tx, None, None, None, None, None, 0, out, ns) == -1
    assert "65 slots, at most 64" in capfd.readouterr().err


def test_product_still_links_nothing_from_the_oracle():
    for p in (qtts.LIB_PATH, qtts.CLI_PATH):
        r = subprocess.run(["ldd", p], capture_output=True, text=True)
        assert "oracle" not in r.stdout and "qtts_ref" not in r.stdout
        data = open(p, "rb").read()
        assert b"orc_talker_step" not in data and b"liboracle" not in data
