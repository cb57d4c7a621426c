"""The lock-step batch GEMV planner (qtts_hip_batch_matvec_plan, host only),
pinned without a GPU: for the decode GEMVs of the 1.7B and 0.6B presets, in
the forms the runtime gives them, and the small shapes of the kernel bars, at
2..64 rows and under the two planner switches, the kernel, its template
integers, grid, block and LDS bytes are those of tests/golden/bgemv_plan.json
(written once from the geometry code of the three kernels before that code was
merged into one planner; running this module as a script rewrites it).  Also
the planner's refusals, and that no planned k_gemvb instantiation is one of
those that spill registers.
"""
import ctypes as C
import json
import os

import pytest

import qtts
from conftest import GOLDEN
from synth_model import PRESETS

STORE, BIAS, BIAS_SILU, RESID, SWIGLU = range(5)
TABLE = os.path.join(GOLDEN, "bgemv_plan.json")
BATCHES = [2, 8, 9, 16, 17, 32, 33, 64]
SWITCHES = {"default": {}, "gemvb_off": {"QTTS_HIP_GEMVB": "0"}, "gb_w8": {"QTTS_HIP_GB_W": "8"}}
SMALL = [(128, 64), (256, 128), (48, 96), (1040, 192)]

PLAIN = dict()
NORMED = dict(norm=True)
SPLITS = {f"kz{kz}_{'self' if s else 'cons'}": dict(epi=RESID, kz=kz, self_reduce=s) for kz in (2, 4) for s in (1, 0)}
QKV = {"normed": NORMED, "normed_p2": dict(norm=True, n_part=2, xcopy="raw"),
       "normed_p4": dict(norm=True, n_part=4, xcopy="raw"), "tabf_sel": dict(src=2, row_sel=True),
       "tab16_normed": dict(norm=True, src=1, xcopy="raw")}
GATE_UP = {"swiglu": dict(norm=True, epi=SWIGLU), "swiglu_p2": dict(norm=True, epi=SWIGLU, n_part=2, xcopy="raw"),
           "swiglu_p4": dict(norm=True, epi=SWIGLU, n_part=4, xcopy="raw"),
           "swiglu_tab16": dict(norm=True, epi=SWIGLU, src=1, row_sel=True)}
RESIDUAL = dict({"resid": dict(epi=RESID)}, **SPLITS)
HEAD = {"normed": NORMED, "normed_copy": dict(norm=True, xcopy="normed")}
SMALL_FORMS = dict({"plain": PLAIN, "normed_copy": dict(norm=True, xcopy="normed"),
                    "resid_rawcopy": dict(epi=RESID, xcopy="raw"), "normed_bias_silu": dict(norm=True, epi=BIAS_SILU),
                    "bias": dict(epi=BIAS), "tab16_normed": dict(norm=True, src=1, xcopy="raw"),
                    "tabf_sel_swiglu": dict(norm=True, epi=SWIGLU, src=2, row_sel=True),
                    "swiglu_p1": dict(norm=True, epi=SWIGLU, n_part=1, xcopy="raw"),
                    "swiglu_p3": dict(norm=True, epi=SWIGLU, n_part=3, xcopy="raw")}, **SPLITS)


def cases():
    """(name, rows, cols, form) of every pinned case"""
    out = []
    for preset in ("1.7b", "0.6b"):
        p = PRESETS[preset]
        roles = [
            ("tk_qkv", (p["NH"] + 2 * p["KV"]) * p["HD"], p["H"], QKV),
            ("tk_o", p["H"], p["NH"] * p["HD"], RESIDUAL),
            ("tk_gate_up", 2 * p["I"], p["H"], GATE_UP),
            ("tk_down", p["H"], p["I"], RESIDUAL),
            ("tk_head", p["V"], p["H"], HEAD),
            ("st_qkv", (p["NHs"] + 2 * p["KVs"]) * p["HDs"], p["Hs"], QKV),
            ("st_o", p["Hs"], p["NHs"] * p["HDs"], RESIDUAL),
            ("st_gate_up", 2 * p["Is"], p["Hs"], GATE_UP),
            ("st_down", p["Hs"], p["Is"], RESIDUAL),
            ("st_lm", p["Vs"], p["Hs"], HEAD),
        ]
        if p["H"] != p["Hs"]:
            roles.append(("st_proj", p["Hs"], p["H"], {"plain": PLAIN, "bias": dict(epi=BIAS)}))
        for role, R, Cc, forms in roles:
            out += [(f"{preset}/{role}/{fn}", R, Cc, f) for fn, f in forms.items()]
    for R, Cc in SMALL:
        out += [(f"small/{R}x{Cc}/{fn}", R, Cc, f) for fn, f in SMALL_FORMS.items()]
    return out


def describe(R, Cc, B, *, norm=False, epi=STORE, src=0, row_sel=False, n_part=0, xcopy=None, kz=0, self_reduce=1,
             **over):
    """the descriptor of a case over stand-in addresses (256-byte aligned, never dereferenced)"""
    d = qtts.BGemvDesc()
    d.rows, d.cols, d.batch, d.A, d.src = R, Cc, B, 1 << 20, src
    if src == 0:
        d.x, d.ldx = 2 << 20, Cc
    else:
        d.table, d.ids, d.ids_bstride, d.ids_rstride, d.ids_off = 3 << 20, 4 << 20, 5, 1, 1
        d.row_sel = (5 << 20) if row_sel else None
    if n_part:
        d.part_in, d.n_part_in = 6 << 20, n_part
    d.norm_w, d.eps = (7 << 20) if norm else None, 1e-6
    d.xcopy = xcopy if isinstance(xcopy, int) else (8 << 20) if xcopy else None   # ("raw" / "normed" / an address)
    d.xcopy_normed = int(xcopy == "normed")
    d.epi, d.bias = epi, (9 << 20) if epi in (BIAS, BIAS_SILU) else None
    d.y, d.ldy = 10 << 20, R // 2 if epi == SWIGLU else R
    d.kz, d.self_reduce, d.part_out = kz, self_reduce, (11 << 20) if kz and not self_reduce else None
    for k, v in over.items():
        setattr(d, k, v)
    return d


def row(plan):
    """a plan as the table holds it: [kernel, template integers, [grid], block, LDS bytes, tpw, cch], or None"""
    if plan is None:
        return None
    return [plan["kernel"], plan["tmpl"], plan["grid"], plan["block"], plan["lds"], plan["tpw"], plan["cch"]]


def plan_table(setenv):
    tab = {}
    for sw, env in SWITCHES.items():
        for k in ("QTTS_HIP_GEMVB", "QTTS_HIP_GB_W"):
            setenv(k, env.get(k))
        for name, R, Cc, form in cases():
            for B in BATCHES:
                tab[f"{name}|{sw}|{B}"] = row(qtts.Kernels.batch_matvec_plan(describe(R, Cc, B, **form)))
    for k in ("QTTS_HIP_GEMVB", "QTTS_HIP_GB_W"):
        setenv(k, None)
    return tab


@pytest.fixture
def setenv(monkeypatch):
    return lambda k, v: monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)


def test_planner_keeps_the_pinned_table(setenv):
    want = json.load(open(TABLE))
    got = plan_table(setenv)
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not diff, (len(diff), list(diff.items())[:5])


def test_table_covers_the_family():
    """every kernel and source kind is planned somewhere, k_gemvm takes over
    with k_gemvb switched off, and every shipped preset shape has a plan at
    every row count under the default switches"""
    tab = json.load(open(TABLE))
    kern = {}
    for k, r in tab.items():
        if r:
            kern.setdefault(r[0], set()).add(r[1][-1])
    assert kern["k_gemvb"] == {0, 1, 2, 3} and kern["k_gemvx"] == {0, 1, 2, 3} and kern["k_gemvm"] >= {0, 1, 2, 3}
    for k, r in tab.items():
        name, sw, B = k.split("|")
        if int(B) > 16:
            assert r is None or r[0] == "k_gemvx", k
        elif sw == "gemvb_off":
            assert r is None or r[0] == "k_gemvm", k
        if sw == "default" and not name.startswith("small/"):
            assert r is not None, k


def test_no_planned_k_gemvb_instantiation_spills():
    """the k_gemvb instantiations whose partials do not fit the registers of a
    1024-thread workgroup (the planner's spills()) are never planned"""
    def spills(SPW, TPW, NBC, PM):
        if PM == 0:
            return False
        if NBC == 16:
            return SPW >= 4
        if SPW == 8:
            return not (TPW == 1 and PM == 2)
        return SPW == 4 and TPW == 3 and PM == 4
    n = 0
    for k, r in json.load(open(TABLE)).items():
        if r and r[0] == "k_gemvb":
            SPW, TPW, NBC, PM, src = r[1]
            assert not spills(SPW, TPW, NBC, PM), (k, r)
            assert (PM > 0) == (src == 1) and TPW * 64 <= r[3], (k, r)
            n += PM > 0
    assert n > 0


# What the planner refuses, next to the nearest arguments it plans: (rows,
# cols, form) refused, the result at 2..16 and at 17..64 rows (1 = not covered,
# -1 = an error: k_gemvm, the last kernel asked at 2..16 rows, reports a bad
# ticket request as an error, the wide kernel does not cover it), then (rows,
# cols, form) planned.
X0, NW0, XC0 = 2 << 20, 7 << 20, 8 << 20
REFUSED = [
    ("rows % 16", (136, 128, PLAIN), 1, 1, (144, 128, PLAIN)),
    ("columns % 32", (128, 144, PLAIN), 1, 1, (128, 160, PLAIN)),
    ("x off 16 bytes", (256, 128, dict(x=X0 + 4)), 1, 1, (256, 128, dict(x=X0 + 16))),
    ("x row stride off 16 bytes", (256, 128, dict(ldx=130)), 1, 1, (256, 128, dict(ldx=132))),
    ("norm weights off 16 bytes", (256, 128, dict(norm=True, norm_w=NW0 + 8)), 1, 1,
     (256, 128, dict(norm=True, norm_w=NW0 + 16))),
    ("copy off 16 bytes", (256, 128, dict(xcopy=XC0 + 4)), 1, 1, (256, 128, dict(xcopy=XC0 + 16))),
    ("split-K with a norm", (256, 128, dict(epi=RESID, kz=2, norm=True)), 1, 1, (256, 128, dict(epi=RESID, kz=2))),
    ("split-K from a table", (256, 128, dict(epi=RESID, kz=2, src=1)), 1, 1, (256, 128, dict(epi=RESID, src=1))),
    ("ticket without the residual epilogue", (256, 128, dict(epi=STORE, kz=2)), -1, 1,
     (256, 128, dict(epi=RESID, kz=2))),
    ("more than 1024 row blocks under a ticket", (16 * 4100, 64, dict(epi=RESID, kz=2)), -1, 1,
     (16 * 4100, 64, dict(epi=RESID, kz=2, self_reduce=0))),
]


@pytest.mark.parametrize("what,bad,rc_small,rc_wide,good", REFUSED, ids=[r[0] for r in REFUSED])
def test_planner_refuses(what, bad, rc_small, rc_wide, good, setenv, capfd):
    lib = qtts.lib()
    for env in SWITCHES.values():
        for k in ("QTTS_HIP_GEMVB", "QTTS_HIP_GB_W"):
            setenv(k, env.get(k))
        for B in BATCHES:
            p = qtts.BGemvPlan()
            rc = lib.qtts_hip_batch_matvec_plan(C.byref(describe(bad[0], bad[1], B, **bad[2])), C.byref(p))
            assert rc == (rc_small if B <= 16 else rc_wide) and p.kernel == 0, (what, B, rc, p.kernel)
            assert qtts.Kernels.batch_matvec_plan(describe(good[0], good[1], B, **good[2])) is not None, (what, B)
    capfd.readouterr()


if __name__ == "__main__":
    def _setenv(k, v):
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    t = plan_table(_setenv)
    with open(TABLE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in t.items())
                + "\n}\n")
    print(len(t), "rows,", sum(v is None for v in t.values()), "not covered")
