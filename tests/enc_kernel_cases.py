"""The cases of the voice-clone encoder kernels' kernel-level tests
(test_gpu_enc_kernels.py, test_enc_kernel_ref.py, test_enc_kernel_abi.py): the
smallest shapes that reach each branch of k_econv's call sites and of
launch_econv's split-K rule, and the inputs of the small kernels.

rows / kz of every case are what launch_econv's rule gives, written out by
hand here; the tests compare them with what the library reports.
"""
from dataclasses import replace

import numpy as np

import enc_kernel_ref as E
from enc_kernel_ref import ACT_GELU, ACT_NONE, ACT_RELU, ACT_RELU_TANH, ACT_SIGMOID, PAD_REFLECT, PAD_REPLICATE, Conv


# ------------------------------------------------------------------ k_econv, generic path
STFT = Conv("stft", 70, 1, 1024, stride=256, padl=384, pmode=PAD_REFLECT, lin=(2000, 1300, 385), lout=(7, 5, 1),
            mono=True, kz=8)
TDNN = Conv("tdnn", 33, 24, 5, padl=2, pmode=PAD_REFLECT, lin=(130, 64, 3), lout=(130, 64, 3), bias=True,
            act_out=ACT_RELU, kz=1)
RES2NET = [Conv(f"res2net-d{d}", 96, 96, 3, dil=d, padl=d, pmode=PAD_REFLECT, lin=(70, 5), lout=(70, 5), x2=True,
                cin=(96, 288), cout=(96, 288), bias=True, act_out=ACT_RELU, kz=2) for d in (2, 4)]
ASP = Conv("asp", 20, 100, 1, lin=(65, 64, 1), lout=(65, 64, 1), bias2=True, act_out=ACT_RELU_TANH, kz=1)
SEANET0 = Conv("seanet-first", 8, 1, 7, padl=6, lin=(200,), lout=(200,), bias=True, kz=1)
RESBLOCK = [Conv("resblock-1", 8, 16, 3, padl=2, lin=(131,), lout=(131,), act_in=1, bias=True, kz=1),
            Conv("resblock-3", 16, 8, 1, lin=(131,), lout=(131,), act_in=1, bias=True, res=True, kz=1)]
STRIDED = [Conv("strided-5", 32, 16, 10, stride=5, padl=5, lin=(203,), lout=(41,), act_in=1, bias=True, kz=1),
           Conv("strided-8", 32, 16, 16, stride=8, padl=8, lin=(130,), lout=(17,), act_in=1, bias=True, kz=2)]
TO_ROWS = Conv("to-rows", 48, 32, 3, padl=2, lin=(9,), lout=(9,), act_in=1, bias=True, tm_out=True, kz=1)
DOWNSAMPLE = Conv("downsample", 48, 48, 4, stride=2, padl=2, pmode=PAD_REPLICATE, lin=(8, 7), lout=(4, 4),
                  tm_in=True, kz=1)
CAP = [Conv("cap-12", 64, 512, 3, padl=2, lin=(40,), lout=(40,), bias=True, kz=12),
       Conv("cap-16", 64, 736, 3, padl=2, lin=(40,), lout=(40,), bias=True, kz=16)]      # nk 69: nk / 4 = 17 > 16
# beyond the call sites: the ELU prologue over the Res2Net sum (the order of the two)
RES2NET_ELU = replace(RES2NET[0], name="res2net-elu", act_in=1, lin=(70,), lout=(70,))

GENERIC = [STFT, TDNN] + RES2NET + [ASP, SEANET0] + RESBLOCK + STRIDED + [TO_ROWS, DOWNSAMPLE] + CAP + [RES2NET_ELU]

# ------------------------------------------------------------------ k_econv, ROWS path (kw 1, time-major)
ROWS_KZ = {64: 1, 40: 1, 256: 2, 288: 2, 512: 4}       # 288: nk 9 over kz 2, uneven
ROWS_EPI = {"none": {}, "gelu": dict(act_out=ACT_GELU), "ls-res": dict(vec=True, res=True)}


def rows_case(K, M, R, epi, **kw):
    return Conv(f"rows-{epi}", M, K, 1, lin=(R,), lout=(R,), tm_in=True, tm_out=True, rows=1, kz=ROWS_KZ.get(K, 1),
                **ROWS_EPI[epi], **kw)


ROWS = [rows_case(K, M, R, epi) for K in ROWS_KZ for M in (48, 130) for R in (1, 63, 65, 130) for epi in ROWS_EPI]
# what the plan must send to the generic kernel: K % 8 != 0, and a row stride that is no multiple of 4
NOT_ROWS = [replace(rows_case(36, 48, 65, "gelu"), name="rows-k36", rows=0),
            replace(rows_case(64, 48, 65, "gelu", xpad=2), name="rows-xt66", rows=0)]

# ------------------------------------------------------------------ the exact-plane instruments
_EXACT_GEOM = [replace(STFT, M=160),
               replace(RES2NET[0], x2=False, bias=False, act_out=ACT_NONE),
               replace(STRIDED[0], act_in=0, bias=False),
               DOWNSAMPLE,
               rows_case(64, 48, 65, "none"),
               rows_case(512, 130, 63, "none")]
EXACT = [replace(g, exact=ins, name=g.name) for g in _EXACT_GEOM for ins in "ABC"]

# beyond the call sites: LayerScale after an activation (the order of the two)
ROWS_GELU_LS = replace(rows_case(64, 48, 65, "gelu", vec=True, res=True), name="rows-gelu-ls")

CASES = GENERIC + ROWS + NOT_ROWS + [ROWS_GELU_LS] + EXACT

# the rows / kz column of the issue's table, by case name (test_enc_kernel_abi.py)
TABLE = {"stft": (0, 8), "tdnn": (0, 1), "res2net-d2": (0, 2), "res2net-d4": (0, 2), "asp": (0, 1),
         "seanet-first": (0, 1), "cap-12": (0, 12), "cap-16": (0, 16), "rows-k36": (0, 1), "rows-xt66": (0, 1)}


def describe(cv, lo, ptr, part=0, part_elems=0):
    """the qtts.EConvDesc of a case; ptr: device address of each buffer of the layout"""
    import qtts
    d = qtts.EConvDesc()
    d.M, d.ci, d.kw, d.stride, d.dil, d.padl, d.pmode, d.act_in = (cv.M, cv.ci, cv.kw, cv.stride, cv.dil, cv.padl,
                                                                   cv.pmode, cv.act_in)
    d.w = ptr["w"]
    d.x = ptr["x"] + 4 * lo["x_off"]
    d.x2 = ptr["x2"] + 4 * lo["x_off"] if cv.x2 else None
    d.xb, d.xc, d.xt = lo["xb"], lo["xc"], lo["xt"]
    for b in range(cv.nb):
        d.lin[b], d.lout[b] = cv.lin[b], cv.lout[b]
    d.nb, d.nmax = cv.nb, cv.nmax
    d.y = ptr["y"] + 4 * lo["y_off"]
    d.yb, d.yc, d.yt = lo["yb"], lo["yc"], lo["yt"]
    d.bias = ptr["bias"] if cv.bias else None
    d.bias2 = ptr["bias2"] if cv.bias2 else None
    d.bias2_b = lo.get("bias2_b", 0)
    d.act_out = cv.act_out
    d.vec = ptr["vec"] if cv.vec else None
    if cv.res:
        d.res, d.rb, d.rc, d.rt = d.y, lo["rb"], lo["rc"], lo["rt"]
    d.part, d.part_elems = (part or None), part_elems
    return d


def host_desc(cv):
    """a descriptor for the host-only plan: aligned dummy addresses, never dereferenced"""
    lo = E.layout(cv, E.reference(cv)[0])
    base = 1 << 20
    return describe(cv, lo, {k: base for k in ("w", "x", "x2", "y", "bias", "bias2", "vec")}), lo


# ------------------------------------------------------------------ small kernels: inputs
STAT_C = (5, 96)
STAT_L = (1, 63, 64, 65, 200)       # ragged in one batch


def stats_inputs(Cn):
    """x [nb][C][200], lens: channel 1 constant, channel 2 mean 100 std 0.01;
    logits spanning +-60, channel 3's raised by 100 (exp of them overflows fp32
    unless the maximum is subtracted first)"""
    rng = E._rng("stats", Cn)
    nb, Lm = len(STAT_L), max(STAT_L)
    x = rng.standard_normal((nb, Cn, Lm)).astype(np.float32)
    x[:, 1, :] = np.float32(0.7)
    x[:, 2, :] = (100.0 + 0.01 * rng.standard_normal((nb, Lm))).astype(np.float32)
    lg = rng.uniform(-60.0, 60.0, (nb, Cn, Lm)).astype(np.float32)
    lg[:, 3, :] = rng.uniform(90.0, 100.0, (nb, Lm)).astype(np.float32)
    lg[:, 0, 0], lg[:, 0, -1] = 60.0, -60.0
    return x, lg, np.array(STAT_L, np.int32)


EGEMV = [(5, 100), (16, 3072), (130, 16)]
EGEMV_ACT = (ACT_NONE, ACT_RELU, ACT_SIGMOID)


def egemv_inputs(R, Cc, nb=3):
    rng = E._rng("egemv", R, Cc)
    return ((rng.standard_normal((R, Cc)) / np.sqrt(Cc)).astype(np.float32),
            rng.standard_normal((nb, Cc)).astype(np.float32), rng.standard_normal(R).astype(np.float32))


LN_D = (64, 100, 512)


def ln_inputs(D, R=5):
    rng = E._rng("ln", D)
    x = rng.standard_normal((R, D)).astype(np.float32)
    x[2] += np.float32(1e3)
    return x, rng.uniform(0.5, 1.5, D).astype(np.float32), rng.standard_normal(D).astype(np.float32), 1e-5


ROPE = [(4, 16), (8, 64)]
ROPE_T = 5


def rope_inputs(nh, hd):
    rng = E._rng("rope", nh, hd)
    x = rng.standard_normal((3 * ROPE_T, nh * hd)).astype(np.float32)
    inv = 1.0 / np.power(10000.0, np.arange(hd // 2) * 2.0 / hd)
    ang = np.arange(ROPE_T)[:, None] * inv[None, :]
    cs = np.concatenate([np.cos(ang), np.cos(ang)], 1).astype(np.float32)
    sn = np.concatenate([np.sin(ang), np.sin(ang)], 1).astype(np.float32)
    return x, cs, sn


MEL = [(513, 128), (513, 5)]
MEL_T = (3, 1)


def mel_inputs(nf, nm):
    """spec [nb][2 nf][3], triangular filters; filter 1 has an empty bin range,
    filter 2 weighs bins whose magnitude keeps its sum under the 1e-5 clamp"""
    rng = E._rng("mel", nf, nm)
    nb, Tm = len(MEL_T), max(MEL_T)
    spec = rng.standard_normal((nb, 2 * nf, Tm)).astype(np.float32)
    fb = np.zeros((nm, nf), np.float32)
    flo, fhi = np.zeros(nm, np.int32), np.zeros(nm, np.int32)
    edges = np.linspace(0, nf, nm + 1).astype(int)
    for m in range(nm):
        lo, hi = edges[m], max(edges[m + 1], edges[m] + 1)
        fb[m, lo:hi] = rng.uniform(0.001, 0.02, hi - lo)
        flo[m], fhi[m] = lo, hi
    flo[1], fhi[1] = 0, 0
    fb[1] = 0
    fb[2] *= np.float32(0.02)
    spec[:, flo[2]:fhi[2], :] *= np.float32(1e-5)
    spec[:, nf + flo[2]:nf + fhi[2], :] *= np.float32(1e-5)
    return spec, fb, flo, fhi, np.array(MEL_T, np.int32)


SE = dict(C=5, lens=(70, 1, 33), Cres=9)     # the residual buffer is wider (9 channels) than the output

RVQ_EXACT = [(1, 1, 2048), (1, 2, 2048), (1, 5, 2048), (2, 3, 100), (1, 5, 100)]     # (nb, T12, CB)
RVQ_RANDOM = [(2, 3, 2048, 15), (1, 5, 100, 33)]                                       # (nb, T12, CB, seed)
