"""The cases of the codec contraction kernels' tests (test_gpu_xgemm.py runs
them on the device, test_xgemm_ref.py checks the bound and the planner on
them without one): the smallest shapes that cross each kernel's own tile,
stage, halo and split boundaries, with the kernel and split count each was
written for."""
from xgemm_ref import (Spec, XA_ROWS, XA_TRANS, XE_STORE, XE_BIAS_N, XE_BIAS_N_GELU, XE_SILU_MUL, XE_SCALE_RESID_N,
                       XE_BIAS_T, XE_BIAS_GAMMA_RES_T, XE_BIAS_M, XE_BIAS_M_RES, XE_BIAS_M_SNAKE, XP_CONVB2,
                       XP_CONVB4, XP_CONV, XP_XLIN, XP_XGEMV, XP_XGEMM, LM, RM)

BM, RES, SNK = XE_BIAS_M, XE_BIAS_M_RES, XE_BIAS_M_SNAKE


def conv(path, M, N, ci, Kw, dil=1, e=BM, force=None, splits=1, **kw):
    return Spec("conv", M, N, ci=ci, Kw=Kw, dil=dil, emode=e, force=path if force is None else force, path=path,
                splits=splits, **kw)


def tconv(path, M, L, ci, k, s, force=None, splits=1, **kw):
    return Spec("tconv", M, L, ci=ci, Kw=k, stride=s, emode=BM, force=path if force is None else force, path=path,
                splits=splits, **kw)


def lin(path, M, N, K, e=XE_STORE, a=XA_ROWS, force=None, splits=1, **kw):
    return Spec("lin", M, N, K=K, emode=e, amode=a, force=path if force is None else force, path=path, splits=splits,
                **kw)


# ---- k_convb<Kw,2>: tile 64 x 128, stages of 16 channels, halo 64 (forced: these
# shapes have too few tiles for the planner to send them there without a workspace)
CONVB2 = [
    conv(XP_CONVB2, 1, 1, 16, 1, bias=False),
    conv(XP_CONVB2, 63, 127, 48, 1),
    conv(XP_CONVB2, 64, 128, 16, 1, e=RES),
    conv(XP_CONVB2, 65, 129, 16, 1, e=SNK, snake=True),
    conv(XP_CONVB2, 64, 200, 16, 1, snake=True),
    conv(XP_CONVB2, 63, 127, 16, 2, 1, hist=True),
    conv(XP_CONVB2, 65, 129, 48, 2, 3, e=RES, snake=True),
    conv(XP_CONVB2, 64, 128, 16, 2, 9, e=SNK),
    conv(XP_CONVB2, 1, 200, 16, 2, 1),
    conv(XP_CONVB2, 64, 1, 16, 2, 3, hist=True),
    conv(XP_CONVB2, 65, 200, 16, 3, 1, hist=True, snake=True),
    conv(XP_CONVB2, 63, 128, 48, 3, 3, e=RES),
    conv(XP_CONVB2, 64, 129, 16, 3, 9, e=SNK, hist=True),
    conv(XP_CONVB2, 1, 127, 16, 3, 1, bias=False),
    conv(XP_CONVB2, 64, 1, 16, 3, 9),
    conv(XP_CONVB2, 1, 200, 16, 7, 1, snake=True),               # the decoder's last conv
    conv(XP_CONVB2, 1, 200, 16, 7, 1, snake=True, hist=True),
    conv(XP_CONVB2, 65, 129, 48, 7, 3, e=SNK, hist=True),
    conv(XP_CONVB2, 63, 127, 16, 7, 9, e=RES, hist=True, snake=True),
    conv(XP_CONVB2, 64, 128, 16, 7, 1, bias=False),
    conv(XP_CONVB2, 64, 1, 16, 7, 9),
    conv(XP_CONVB2, 65, 129, 16, 7, 3, hist=True, planted=True),
    conv(XP_CONVB2, 64, 128, 48, 1, planted=True),
    conv(XP_CONVB2, 63, 200, 16, 3, 9, planted=True, bias=False),
    conv(XP_CONVB2, 65, 127, 48, 2, 1, hist=True, planted=True),
    # halo 66 > 64: the planner must send it to the generic kernel
    conv(XP_XGEMM, 65, 129, 16, 7, 11, force=-1),
    conv(XP_XGEMM, 65, 129, 16, 7, 11, force=-1, hist=True, snake=True, e=SNK),
]

# ---- k_convb<Kw,4>: tile 64 x 256
CONVB4 = [
    conv(XP_CONVB4, 64, 255, 16, 1),
    conv(XP_CONVB4, 65, 256, 16, 7, 3, hist=True),
    conv(XP_CONVB4, 64, 257, 16, 7, 1, snake=True, e=SNK),
    conv(XP_CONVB4, 65, 257, 48, 1, e=RES),
    conv(XP_CONVB4, 65, 257, 16, 7, 9, planted=True),
    conv(XP_CONVB4, 64, 256, 48, 1, planted=True, bias=False),
]

# ---- k_conv<Kw>: fp32 MFMA, same tiles as k_convb<Kw,2>, with a prologue
CONV = [
    conv(XP_CONV, 1, 1, 16, 1, snake=True),
    conv(XP_CONV, 63, 127, 48, 1, snake=True),
    conv(XP_CONV, 65, 129, 16, 1, e=RES, snake=True),
    conv(XP_CONV, 64, 128, 16, 7, 3, snake=True, hist=True),
    conv(XP_CONV, 65, 200, 48, 7, 9, e=SNK, snake=True),
    conv(XP_CONV, 1, 200, 16, 7, 1, snake=True, hist=True),
    conv(XP_CONV, 64, 1, 16, 7, 9, snake=True, bias=False),
    conv(XP_CONV, 64, 128, 16, 1, e=SNK, snake=True),
    conv(XP_CONV, 64, 200, 48, 1, snake=True),
    conv(XP_CONV, 63, 127, 16, 7, 1, snake=True),
    conv(XP_CONV, 65, 129, 16, 7, 3, e=RES, snake=True, hist=True),
]

# ---- input-channel splits (k_conv_reduce applies the epilogue): 64 channels make 2, 128 make 4
_W = 65 * 129
SPLIT = [
    conv(XP_CONVB2, 65, 129, 64, 7, 1, splits=2, part=2 * _W),
    conv(XP_CONVB2, 65, 129, 128, 1, e=RES, splits=4, part=4 * _W),
    conv(XP_CONVB2, 65, 129, 64, 3, 3, e=SNK, hist=True, snake=True, splits=2, part=2 * _W),
    conv(XP_CONVB2, 65, 129, 64, 7, 1, splits=2, part=2 * _W, planted=False, bias=False),
    conv(XP_CONV, 65, 129, 64, 1, snake=True, splits=2, part=2 * _W),
    conv(XP_CONV, 65, 129, 128, 7, 1, e=RES, snake=True, splits=4, part=4 * _W),
    conv(XP_CONV, 65, 129, 64, 2, 1, e=SNK, snake=True, hist=True, splits=2, part=2 * _W),
    conv(XP_CONVB4, 65, 257, 64, 1, splits=2, part=2 * 65 * 257),
    conv(XP_CONVB4, 65, 257, 128, 7, 3, e=SNK, hist=True, splits=4, part=4 * 65 * 257),
    # the planner's own choice: a workspace that allows >= 2 splits brings the conv kernels in
    conv(XP_CONVB2, 65, 129, 64, 7, 1, force=-1, splits=2, part=2 * _W, seed=1),
    # one element too small for 2 splits: 1 split; unforced, the conv kernels are out (K = 448: no split-K either)
    conv(XP_CONVB2, 65, 129, 64, 7, 1, splits=1, part=2 * _W - 1, seed=2),
    conv(XP_XGEMM, 65, 129, 64, 7, 1, force=-1, splits=1, part=2 * _W - 1, seed=3),
]

# ---- transposed convs through tconv_run
TCONV = [
    # all phases (x splits) in grid z of one conv-kernel launch
    tconv(XP_CONVB2, 65, 129, 64, 4, 2, force=-1, splits=2, part=2 * 2 * 65 * 129),
    tconv(XP_CONVB2, 63, 129, 64, 16, 8, force=-1, splits=2, part=2 * 8 * 63 * 129, hist=True),
    tconv(XP_CONVB2, 65, 1, 64, 6, 3, force=-1, splits=2, part=2 * 3 * 65, snake=True),
    tconv(XP_CONVB2, 63, 129, 64, 5, 5, force=-1, splits=2, part=2 * 5 * 63 * 129),
    tconv(XP_CONVB2, 63, 129, 16, 2, 2),
    tconv(XP_CONVB2, 65, 1, 16, 5, 5, bias=False),
    tconv(XP_CONVB2, 65, 129, 16, 6, 3, snake=True, hist=True),
    tconv(XP_CONVB2, 63, 1, 16, 16, 8, hist=True),
    tconv(XP_CONVB2, 65, 129, 16, 4, 2, planted=True, hist=True),
    tconv(XP_CONVB2, 63, 129, 16, 16, 8, planted=True),
    tconv(XP_CONVB4, 65, 129, 16, 4, 2),
    tconv(XP_CONVB4, 63, 129, 64, 6, 3, splits=2, part=2 * 3 * 63 * 129, hist=True, snake=True),
    tconv(XP_CONV, 65, 129, 64, 4, 2, splits=2, part=2 * 2 * 65 * 129, snake=True),
    tconv(XP_CONV, 65, 129, 16, 16, 8, snake=True, hist=True),
    tconv(XP_CONV, 63, 1, 16, 2, 2, snake=True),
    # one k_xgemm per phase: 12 channels make no whole stage; 16 channels without a workspace too few tiles
    tconv(XP_XGEMM, 63, 129, 12, 4, 2, force=-1),
    tconv(XP_XGEMM, 65, 1, 12, 16, 8, force=-1, hist=True),
    tconv(XP_XGEMM, 65, 129, 12, 6, 3, force=-1, snake=True, hist=True),
    tconv(XP_XGEMM, 63, 129, 12, 5, 5, force=-1, bias=False),
    tconv(XP_XGEMM, 65, 129, 16, 2, 2, force=-1),
    tconv(XP_XGEMM, 63, 129, 64, 4, 2, force=XP_XGEMM, snake=True),
]

# ---- k_xgemm: tile 64 x 64, K steps of 32
XGEMM = [
    lin(XP_XGEMM, 1, 65, 15),
    lin(XP_XGEMM, 63, 64, 32, e=XE_BIAS_N, a=XA_TRANS),
    lin(XP_XGEMM, 64, 63, 33, e=XE_BIAS_N_GELU),
    lin(XP_XGEMM, 65, 1, 33, e=XE_BIAS_T, a=XA_TRANS),
    lin(XP_XGEMM, 64, 64, 32),
    lin(XP_XGEMM, 65, 65, 15, e=XE_SILU_MUL, a=XA_TRANS),
    lin(XP_XGEMM, 1, 1, 33, e=XE_SCALE_RESID_N),
    lin(XP_XGEMM, 63, 65, 32, e=XE_BIAS_GAMMA_RES_T),
    conv(XP_XGEMM, 63, 65, 5, 3, 2),
    conv(XP_XGEMM, 65, 63, 11, 3, 1, e=RES, snake=True, hist=True),
    conv(XP_XGEMM, 64, 64, 32, 1, e=SNK),
    conv(XP_XGEMM, 1, 1, 16, 2, 1, hist=True),
    # split-K through k_xg_reduce: z ranges of >= 8 K steps
    lin(XP_XGEMM, 65, 63, 512, e=XE_BIAS_N, a=XA_TRANS, splits=2, part=2 * 65 * 63),
    lin(XP_XGEMM, 63, 65, 1000, e=XE_SCALE_RESID_N, splits=3, part=3 * 63 * 65),
    lin(XP_XGEMM, 64, 64, 1024, e=XE_BIAS_N_GELU, splits=4, part=4 * 64 * 64),
    conv(XP_XGEMM, 65, 63, 80, 7, 2, e=RES, hist=True, splits=2, part=2 * 65 * 63),
    lin(XP_XGEMM, 65, 63, 512, e=XE_BIAS_T, a=XA_TRANS, splits=1, part=2 * 65 * 63 - 1),
]

# ---- k_xlin: tile 64 x 64, stages of 128 K, every linear epilogue
XLIN = [
    lin(XP_XLIN, 5, 64, 128),
    lin(XP_XLIN, 63, 192, 384, e=XE_BIAS_N, splits=2, part=2 * 63 * 192),          # 3 stages on 2 splits
    lin(XP_XLIN, 64, 64, 384, e=XE_BIAS_N_GELU, splits=3, part=3 * 64 * 64),       # one split per stage
    lin(XP_XLIN, 65, 192, 128, e=XE_SILU_MUL),
    lin(XP_XLIN, 130, 64, 384, e=XE_SCALE_RESID_N, splits=2, part=2 * 130 * 64),
    lin(XP_XLIN, 63, 64, 128, e=XE_BIAS_T),
    lin(XP_XLIN, 65, 192, 384, e=XE_BIAS_GAMMA_RES_T, splits=3, part=3 * 65 * 192),
    lin(XP_XLIN, 130, 192, 384, e=XE_BIAS_N),
    lin(XP_XLIN, 5, 192, 384, e=XE_SILU_MUL, splits=3, part=3 * 5 * 192),
    lin(XP_XLIN, 64, 192, 128, e=XE_SCALE_RESID_N),
    lin(XP_XLIN, 65, 64, 384, e=XE_BIAS_T, splits=2, part=2 * 65 * 64),
    lin(XP_XLIN, 63, 64, 128, e=XE_BIAS_GAMMA_RES_T),
    lin(XP_XLIN, 130, 64, 128, e=XE_BIAS_N_GELU),
    lin(XP_XLIN, 64, 192, 128, planted=True),
    lin(XP_XLIN, 65, 64, 128, e=XE_BIAS_T, planted=True),
    lin(XP_XLIN, 63, 64, 384, planted=True, splits=3, part=3 * 63 * 64),
    # shapes the predicate rejects: the planner reports another kernel
    lin(XP_XGEMM, 64, 65, 128, force=-1),
    lin(XP_XGEMM, 64, 64, 130, force=-1),
    lin(XP_XGEMM, 64, 64, 128, force=-1, lda=129),
]
XLIN_REJECTED = [s for s in XLIN if s.path == XP_XGEMM]

# ---- k_xgemv: <= 4 rows, 32 slots x 8 lanes, K slots so that the grid holds >= 512 workgroups
XGEMV = [
    lin(XP_XGEMV, 1, 1, 256, splits=8, force=-1),
    lin(XP_XGEMV, 2, 33, 512, e=XE_BIAS_N, a=XA_TRANS, splits=16, force=-1),
    lin(XP_XGEMV, 3, 600, 3840, e=XE_BIAS_N_GELU, splits=8, force=-1),
    lin(XP_XGEMV, 4, 20000, 256, e=XE_SILU_MUL, a=XA_TRANS, splits=1, force=-1),
    lin(XP_XGEMV, 4, 20000, 512, e=XE_SCALE_RESID_N, splits=1, force=-1),
    lin(XP_XGEMV, 1, 600, 3840, e=XE_BIAS_T, a=XA_TRANS, splits=8, force=-1),
    lin(XP_XGEMV, 2, 600, 256, e=XE_BIAS_GAMMA_RES_T, splits=8, force=-1),
    lin(XP_XGEMV, 3, 1, 3840, splits=8, force=-1),        # 120 blocks of 32: 16 slots would not divide them
    lin(XP_XGEMV, 4, 33, 256, a=XA_TRANS, splits=8, force=-1),
    lin(XP_XGEMV, 3, 33, 512, e=XE_BIAS_N, splits=16),
    # 4 rows of 4096 do not fit the LDS test
    lin(XP_XGEMM, 2, 33, 4096, force=-1),
]

CASES = CONVB2 + CONVB4 + CONV + SPLIT + TCONV + XGEMM + XLIN + XGEMV
# forcing a kernel on a shape it was not written for: 1, nothing launched
REFUSED = [
    conv(XP_CONVB2, 65, 129, 16, 7, 11, hist=True),     # halo 66
    conv(XP_CONVB4, 64, 128, 12, 1),                     # no whole channel stage
    conv(XP_CONV, 64, 128, 16, 5, 1),                    # no 5-tap instantiation
    conv(XP_XLIN, 64, 128, 16, 1),
    conv(XP_XGEMV, 4, 128, 16, 1),
    tconv(XP_CONVB2, 63, 129, 12, 4, 2),
    tconv(XP_XLIN, 63, 129, 16, 4, 2),
    lin(XP_XLIN, 64, 65, 128),
    lin(XP_XLIN, 64, 64, 130),
    lin(XP_XLIN, 64, 64, 128, lda=129),
    lin(XP_XLIN, 4, 64, 128),
    lin(XP_XGEMV, 5, 64, 256),
    lin(XP_XGEMV, 2, 33, 4096),
    lin(XP_XGEMV, 2, 33, 250),
    lin(XP_CONVB2, 64, 64, 128),
]


# ---- every contraction of a 1.7B decode of T frames (tools/synth_model.py "1.7b":
# c_latent 1024, c_hidden 1024, c_cbdim 512, c_inter 3072, c_dec 1536, rates 8 5 4 3),
# with the model's workspace, under the planner's own choice
MODEL_PART = 8 << 20
LAT, HID, CBD, INTER, DEC, RATES = 1024, 1024, 512, 3072, 1536, (8, 5, 4, 3)


def shipped(T):
    """[(name, Spec without path / splits)] in decode order, duplicates dropped"""
    S = [("pre_conv", conv(-1, LAT, T, CBD, 3, part=MODEL_PART)),
         ("input_proj", lin(-1, T, HID, LAT, e=XE_BIAS_N, a=XA_TRANS, part=MODEL_PART)),
         ("q/k/v_proj", lin(-1, T, HID, HID, part=MODEL_PART)),
         ("o_proj", lin(-1, T, HID, HID, e=XE_SCALE_RESID_N, part=MODEL_PART)),
         ("gate_proj", lin(-1, T, INTER, HID, part=MODEL_PART)),
         ("up_proj", lin(-1, T, INTER, HID, e=XE_SILU_MUL, part=MODEL_PART)),
         ("down_proj", lin(-1, T, HID, INTER, e=XE_SCALE_RESID_N, part=MODEL_PART)),
         ("output_proj", lin(-1, T, LAT, HID, e=XE_BIAS_T, part=MODEL_PART))]
    L = T
    for s in range(2):
        S.append((f"upsample.{s}.tconv", tconv(-1, LAT, L, LAT, 2, 2, part=MODEL_PART)))
        L *= 2
        S.append((f"upsample.{s}.pwconv1", lin(-1, L, 4 * LAT, LAT, e=XE_BIAS_N_GELU, part=MODEL_PART)))
        S.append((f"upsample.{s}.pwconv2", lin(-1, L, LAT, 4 * LAT, e=XE_BIAS_GAMMA_RES_T, part=MODEL_PART)))
    S.append(("decoder.0", conv(-1, DEC, L, LAT, 7, part=MODEL_PART)))
    for b, r in enumerate(RATES):
        ci, co = DEC >> b, DEC >> (b + 1)
        S.append((f"decoder.{b + 1}.tconv", tconv(-1, co, L, ci, 2 * r, r, snake=True, part=MODEL_PART)))
        L *= r
        for d in (1, 3, 9):
            S.append((f"decoder.{b + 1}.res.d{d}.conv1", conv(-1, co, L, co, 7, d, e=SNK, snake=True, part=MODEL_PART)))
            S.append((f"decoder.{b + 1}.res.d{d}.conv2", conv(-1, co, L, co, 1, e=RES, part=MODEL_PART)))
    S.append(("decoder.6", conv(-1, 1, L, DEC // 16, 7, snake=True, part=MODEL_PART)))
    out, seen = [], set()
    for name, sp in S:
        sp = Spec(**{**sp.__dict__, "force": -1})
        if sp not in seen:
            seen.add(sp)
            out.append((name, sp))
    return out


C2, C4, XL, GV, GM = XP_CONVB2, XP_CONVB4, XP_XLIN, XP_XGEMV, XP_XGEMM
# the hot path's choices for a 1.7B decode with the model's 8 Mi-float workspace:
# (kernel, splits) per contraction, in decode order
SHIPPED = {
    1: [("pre_conv", C2, 16), ("input_proj", GV, 16), ("q/k/v_proj", GV, 16), ("o_proj", GV, 16), ("gate_proj", GV, 8),
        ("up_proj", GV, 8), ("down_proj", GV, 16), ("output_proj", GV, 16), ("upsample.0.tconv", C4, 32),
        ("upsample.0.pwconv1", GV, 4), ("upsample.0.pwconv2", GM, 16), ("upsample.1.tconv", C4, 32),
        ("upsample.1.pwconv1", GV, 4), ("upsample.1.pwconv2", GM, 16), ("decoder.0", C4, 32),
        ("decoder.1.tconv", C4, 8), ("decoder.1.res.d1.conv1", C2, 16), ("decoder.1.res.d1.conv2", C2, 16),
        ("decoder.1.res.d3.conv1", C2, 16), ("decoder.1.res.d9.conv1", C2, 16), ("decoder.2.tconv", C2, 16),
        ("decoder.2.res.d1.conv1", C2, 8), ("decoder.2.res.d1.conv2", C2, 8), ("decoder.2.res.d3.conv1", C2, 8),
        ("decoder.2.res.d9.conv1", C2, 8), ("decoder.3.tconv", C2, 8), ("decoder.3.res.d1.conv1", C2, 4),
        ("decoder.3.res.d1.conv2", C2, 4), ("decoder.3.res.d3.conv1", C2, 4), ("decoder.3.res.d9.conv1", C2, 4),
        ("decoder.4.tconv", C2, 4), ("decoder.4.res.d1.conv1", C2, 2), ("decoder.4.res.d1.conv2", C2, 2),
        ("decoder.4.res.d3.conv1", C2, 2), ("decoder.4.res.d9.conv1", C2, 2), ("decoder.6", C2, 2)],
    16: [("pre_conv", C2, 16), ("input_proj", GM, 4), ("q/k/v_proj", XL, 8), ("o_proj", XL, 8), ("gate_proj", XL, 6),
         ("up_proj", XL, 6), ("down_proj", XL, 16), ("output_proj", XL, 8), ("upsample.0.tconv", C4, 32),
         ("upsample.0.pwconv1", XL, 4), ("upsample.0.pwconv2", XL, 16), ("upsample.1.tconv", C4, 32),
         ("upsample.1.pwconv1", XL, 4), ("upsample.1.pwconv2", XL, 16), ("decoder.0", C4, 32),
         ("decoder.1.tconv", C4, 8), ("decoder.1.res.d1.conv1", C2, 16), ("decoder.1.res.d1.conv2", C2, 16),
         ("decoder.1.res.d3.conv1", C2, 16), ("decoder.1.res.d9.conv1", C2, 16), ("decoder.2.tconv", C2, 8),
         ("decoder.2.res.d1.conv1", C2, 8), ("decoder.2.res.d1.conv2", C2, 8), ("decoder.2.res.d3.conv1", C2, 8),
         ("decoder.2.res.d9.conv1", C2, 8), ("decoder.3.tconv", C2, 4), ("decoder.3.res.d1.conv1", C2, 4),
         ("decoder.3.res.d1.conv2", C2, 4), ("decoder.3.res.d3.conv1", C2, 4), ("decoder.3.res.d9.conv1", C2, 4),
         ("decoder.4.tconv", C2, 2), ("decoder.4.res.d1.conv1", C2, 2), ("decoder.4.res.d1.conv2", C2, 2),
         ("decoder.4.res.d3.conv1", C2, 2), ("decoder.4.res.d9.conv1", C2, 2), ("decoder.6", C2, 2)],
    128: [("pre_conv", C2, 16), ("input_proj", GM, 4), ("q/k/v_proj", XL, 8), ("o_proj", XL, 8), ("gate_proj", XL, 3),
          ("up_proj", XL, 3), ("down_proj", XL, 8), ("output_proj", XL, 8), ("upsample.0.tconv", C4, 32),
          ("upsample.0.pwconv1", XL, 1), ("upsample.0.pwconv2", XL, 4), ("upsample.1.tconv", C4, 16),
          ("upsample.1.pwconv1", XL, 1), ("upsample.1.pwconv2", XL, 2), ("decoder.0", C2, 8),
          ("decoder.1.tconv", C2, 2), ("decoder.1.res.d1.conv1", C2, 2), ("decoder.1.res.d1.conv2", C2, 2),
          ("decoder.1.res.d3.conv1", C2, 2), ("decoder.1.res.d9.conv1", C2, 2), ("decoder.2.tconv", C2, 1),
          ("decoder.2.res.d1.conv1", C2, 1), ("decoder.2.res.d1.conv2", C2, 1), ("decoder.2.res.d3.conv1", C2, 1),
          ("decoder.2.res.d9.conv1", C2, 1), ("decoder.3.tconv", C4, 1), ("decoder.3.res.d1.conv1", C4, 1),
          ("decoder.3.res.d1.conv2", C4, 1), ("decoder.3.res.d3.conv1", C4, 1), ("decoder.3.res.d9.conv1", C4, 1),
          ("decoder.4.tconv", C4, 1), ("decoder.4.res.d1.conv1", C4, 1), ("decoder.4.res.d1.conv2", C4, 1),
          ("decoder.4.res.d3.conv1", C4, 1), ("decoder.4.res.d9.conv1", C4, 1), ("decoder.6", C4, 1)],
}


# ---- the buffers of a case and its C description
def layout(sp):
    """leading dimensions and buffer shapes: every row is longer than its data"""
    K, t_mode = sp.kdim, sp.emode in (XE_BIAS_T, XE_BIAS_GAMMA_RES_T)
    lo = {"ldc": (sp.M if t_mode else sp.ncol) + 5, "crows": (sp.N if t_mode else sp.M) + 2, "ldaux": sp.N + 3}
    if sp.kind == "lin":
        lo["lda"] = sp.lda or (K + 4 if sp.amode == XA_ROWS else sp.M + 3)
        lo["ldb"] = K + 4
    else:
        lo["lda"] = K if sp.kind == "conv" else 0
        lo["ldb"] = LM + sp.N + RM
    return lo


def describe(sp, ptr):
    """qtts.XGemmDesc of a case; ptr: name -> device address (A, B = the input's
    column 0, C, and whichever of sa sb bias vec aux ea eb the case has)"""
    import qtts
    lo = layout(sp)
    d = qtts.XGemmDesc()
    d.M, d.N, d.K = sp.M, sp.N, sp.kdim
    d.amode = sp.amode if sp.kind == "lin" else (XA_ROWS if sp.kind == "conv" else 2)
    d.bmode = {"lin": 0, "conv": 1, "tconv": 2}[sp.kind]
    d.emode = sp.emode
    d.A, d.lda, d.B, d.ldb = ptr["A"], lo["lda"], ptr["B"], lo["ldb"]
    d.Kw, d.dil, d.stride, d.L, d.tmin = sp.Kw, sp.dil, sp.stride, sp.N, sp.tmin
    d.pad = sp.halo if sp.kind == "conv" else 0
    d.co = sp.M if sp.kind == "tconv" else 0
    d.C, d.ldc = ptr["C"], lo["ldc"]
    for k in ("sa", "sb", "bias", "vec", "aux", "ea", "eb"):
        setattr(d, k, ptr.get(k))
    d.ldaux = lo["ldaux"]
    if sp.emode in (XE_SCALE_RESID_N, XE_BIAS_M_RES, XE_BIAS_GAMMA_RES_T):
        d.res, d.ldres = ptr["C"], lo["ldc"]         # the codec's in-place forms
    return d


def fake_ptrs(sp):
    """16-byte aligned stand-ins for a planner-only query (nothing is dereferenced)"""
    p = {k: 4096 * (i + 1) for i, k in enumerate(("A", "B", "C", "bias", "vec", "aux", "ea", "eb"))}
    if sp.snake:
        p["sa"], p["sb"] = 4096 * 20, 4096 * 21
    return p
