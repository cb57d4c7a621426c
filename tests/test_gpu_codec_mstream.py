"""The multi-stream exact streaming codec (qwen_tts_codec_mstream_*): n
independent causal states decoded in one launch sequence per push.

Bounds are the single stream's (test_gpu_model.py::test_codec_stream_equals_
full_decode): 1e-5 max-abs against the full decode of the same codes on the
device, and audio_close (1e-4) against the oracle.  The kernel-level part runs
the conv forms' stream axis (qtts_hip_xgemm_seg_case) against the float64
reference and bound of xgemm_ref.py, per segment, with no constant of its own.
"""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import qtts
import xgemm_ref as X
from xgemm_cases import describe, layout

pytestmark = pytest.mark.gpu

_ip, _fp = C.POINTER(C.c_int), C.POINTER(C.c_float)


def audio_close(a, ref):
    assert a is not None and a.shape == ref.shape, (None if a is None else a.shape, ref.shape)
    mse = float(np.mean((a.astype(np.float64) - ref) ** 2)) if len(ref) else 0.0
    assert mse < 1e-4, mse
    if len(ref):
        assert np.abs(a - ref).max() < 1e-4, np.abs(a - ref).max()


_CODES, _FULL = {}, {}


def codes_of(n, T):
    """[n, T, 16] random codes, fixed per (n, T)"""
    if (n, T) not in _CODES:
        c = np.random.default_rng(1000 + 97 * n + T).integers(0, 2048, size=(n, T, 16)).astype(np.int32)
        c.setflags(write=False)
        _CODES[(n, T)] = c
    return _CODES[(n, T)]


def full_decode(m, codes):
    """codec_decode of one stream's codes, computed once per code array"""
    key = codes.tobytes()
    if key not in _FULL:
        a = m.codec_decode(np.ascontiguousarray(codes))
        a.setflags(write=False)
        _FULL[key] = a
    return _FULL[key]


def split(codes, sched):
    """[n, T, 16] -> per stream the list of chunks of the schedule"""
    assert sum(sched) == codes.shape[1]
    cuts = np.cumsum([0] + list(sched))
    return [[codes[s, cuts[i]:cuts[i + 1]] for i in range(len(sched))] for s in range(codes.shape[0])]


def run(m, codes, sched):
    outs = m.codec_mstream(split(codes, sched))
    for s in range(codes.shape[0]):
        assert [len(o) for o in outs[s]] == [1920 * t for t in sched]
    return [np.concatenate(o) for o in outs]


SCHED_A, SCHED_B = [1, 3, 7, 16, 23], [1, 40, 16, 5, 88]


# ---------------------------------------------------------------- 1. equals the full decode
@pytest.mark.parametrize("n,sched", [(1, SCHED_A), (3, SCHED_A), (17, SCHED_A), (3, SCHED_B)],
                         ids=["n1-T50", "n3-T50", "n17-T50", "n3-T150"])
def test_every_stream_equals_its_full_decode(tts_tiny, oracle, n, sched):
    codes = codes_of(n, sum(sched))
    got = run(tts_tiny, codes, sched)
    worst = 0.0
    for s in range(n):
        full = full_decode(tts_tiny, codes[s])
        assert got[s].shape == full.shape
        worst = max(worst, float(np.abs(got[s] - full).max()))
    print(f"measured  n={n} T={sum(sched)}: largest |stream - full decode| {worst:.3e}")
    assert worst < 1e-5, worst
    for s in range(n):
        audio_close(got[s], oracle.codec_decode(codes[s]))


@pytest.mark.parametrize("n", [2, 3])
def test_stacked_rows_on_the_gemv_and_bf16_linear_kernels(gpu, n):
    """the tiny codec's 64-wide linears all run on the generic kernel; with
    256-wide ones (the shipped codec's are 1024) the stacked rows of a push go
    through k_xgemv at n T <= 4 rows -- its transposed input and outputs split
    over the planes -- and through k_xlin above that"""
    from conftest import model_dir
    m = qtts.QwenTTS(model_dir("tiny", c_hidden=256, c_latent=256, c_cbdim=128, c_inter=512))
    try:
        sched = [1, 1, 2, 4, 3]
        codes = codes_of(n, sum(sched))
        got = run(m, codes, sched)
        for s in range(n):
            full = m.codec_decode(np.ascontiguousarray(codes[s]))
            assert got[s].shape == full.shape
            d = float(np.abs(got[s] - full).max())
            assert d < 1e-5, (s, d)
        single = np.concatenate(m.codec_stream(split(codes, sched)[0]))
        assert np.abs(single - got[0]).max() < 1e-5
    finally:
        m.close()


# ---------------------------------------------------------------- 2. no crosstalk
def test_a_stream_does_not_see_its_neighbours(tts_tiny):
    codes = codes_of(3, 50)
    a = run(tts_tiny, codes, SCHED_A)
    other = codes.copy()
    other[0] = codes_of(1, 50)[0]
    other[2] = (codes[2] + 1) % 2048
    b = run(tts_tiny, other, SCHED_A)
    np.testing.assert_array_equal(a[1], b[1])
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[2], b[2])


# ---------------------------------------------------------------- 3. subsets and the ragged tail
def test_subsets_and_a_short_tail(tts_tiny):
    m = tts_tiny
    codes = codes_of(3, 24)
    assert m.codec_mstream_begin(3, 64) == 0
    out = [[], [], []]

    def push(streams, t0, T):
        o = m.codec_mstream_push(streams, np.stack([codes[s, t0:t0 + T] for s in streams]))
        assert o is not None
        for s, a in zip(streams, o):
            out[s].append(a)

    for k in range(3):
        push([0, 1, 2], 4 * k, 4)
    push([1], 12, 1)
    push([0, 2], 12, 4)
    push([0, 2], 16, 8)
    assert [m.codec_mstream_pos(s) for s in range(3)] == [24, 13, 24]
    assert m.codec_mstream_pos(3) == -1 and m.codec_mstream_pos(-1) == -1
    for s, T in ((0, 24), (1, 13), (2, 24)):
        got = np.concatenate(out[s])
        full = full_decode(m, codes[s, :T])
        assert got.shape == full.shape
        assert np.abs(got - full).max() < 1e-5, (s, np.abs(got - full).max())


# ---------------------------------------------------------------- 4. reuse, and the single stream beside it
def test_begin_again_and_the_other_codec_paths_in_between(tts_tiny):
    m = tts_tiny
    codes = codes_of(3, 50)
    first = run(m, codes, SCHED_A)
    again = run(m, codes, SCHED_A)
    for s in range(3):
        np.testing.assert_array_equal(first[s], again[s])
    single = np.concatenate(m.codec_stream([c for c in split(codes, SCHED_A)[0]]))
    assert np.abs(single - full_decode(m, codes[0])).max() < 1e-5
    m.codec_decode(np.ascontiguousarray(codes_of(1, 150)[0]))      # a longer decode: the codec state is re-allocated
    third = run(m, codes, SCHED_A)
    for s in range(3):
        np.testing.assert_array_equal(first[s], third[s])


# ---------------------------------------------------------------- 5. refusals
def _raw_push(m, streams, T, n=None):
    """qwen_tts_codec_mstream_push as given (no checks on this side): the return value"""
    st = np.asarray(streams, np.int32)
    n = len(st) if n is None else n
    k = max(len(st), 1)
    st = np.ascontiguousarray(np.resize(st, k) if len(st) else np.zeros(1, np.int32))
    codes = np.zeros((k, max(T, 1), 16), np.int32)
    outs = [np.full(max(T, 1) * 1920, 7.0, np.float32) for _ in range(k)]
    po = (_fp * k)(*[o.ctypes.data_as(_fp) for o in outs])
    rc = qtts.lib().qwen_tts_codec_mstream_push(m.ctx, n, st.ctypes.data_as(_ip), codes.ctypes.data_as(_ip), T, po)
    if rc < 0:
        assert all(np.all(o == 7.0) for o in outs)      # nothing was written
    return rc


def test_refusals_leave_the_streams_untouched(tts_tiny, tiny_dir):
    m = tts_tiny
    codes = codes_of(3, 24)

    def sequence(disturb):
        assert m.codec_mstream_begin(3, 16) == 0
        a = m.codec_mstream_push([0, 1, 2], codes[:, :2])
        if disturb:
            assert _raw_push(m, [], 1, n=0) == -1                 # bad n
            assert _raw_push(m, [0, 1, 2, 0], 1, n=4) == -1       # more streams than begun
            assert _raw_push(m, [0, 3], 1) == -1                  # index out of range
            assert _raw_push(m, [-1], 1) == -1
            assert _raw_push(m, [1, 1], 1) == -1                  # listed twice
            assert _raw_push(m, [0, 1], 0) == -1                  # T < 1
            assert _raw_push(m, [0, 1], -3) == -1
            assert _raw_push(m, [0, 1, 2], 15) == -1              # 2 + 15 > max_frames 16
        b = m.codec_mstream_push([1], codes[1:2, 2:3])
        if disturb:
            assert _raw_push(m, [0, 1], 1) == -1                  # positions 2 and 3
            assert _raw_push(m, [1, 2], 2) == -1
            assert [m.codec_mstream_pos(s) for s in range(3)] == [2, 3, 2]
        c = m.codec_mstream_push([0, 2], codes[[0, 2], 2:6])
        d = m.codec_mstream_push([1], codes[1:2, 3:6])
        e = m.codec_mstream_push([0, 1, 2], codes[:, 6:16])       # exactly to max_frames
        assert None not in (a, b, c, d, e)
        if disturb:
            assert _raw_push(m, [0], 1) == -1                     # full
        return [np.concatenate(x) for x in (a, b, c, d, e)]

    clean = sequence(False)
    disturbed = sequence(True)
    for x, y in zip(clean, disturbed):
        np.testing.assert_array_equal(x, y)
    # a push without begin: a context that never began a multi-stream
    fresh = qtts.QwenTTS(tiny_dir)
    try:
        assert _raw_push(fresh, [0], 1) == -1
        assert fresh.codec_mstream_pos(0) == -1
        assert fresh.codec_mstream_begin(0, 16) == -1 and fresh.codec_mstream_begin(65, 16) == -1
        assert fresh.codec_mstream_begin(2, 0) == -1
        assert _raw_push(fresh, [0], 1) == -1
    finally:
        fresh.close()


# ---------------------------------------------------------------- 6. the conv forms' stream axis, kernel level
M_ROWS = 65                      # two row tiles
BASES = {
    "k7d1": dict(kind="conv", ci=32, Kw=7, dil=1, hist=True, emode=X.XE_BIAS_M),
    "k7d9-snake": dict(kind="conv", ci=32, Kw=7, dil=9, hist=True, snake=True, emode=X.XE_BIAS_M_SNAKE),
    "k3": dict(kind="conv", ci=32, Kw=3, dil=1, hist=True, emode=X.XE_BIAS_M),
    "k1-res": dict(kind="conv", ci=32, Kw=1, dil=1, emode=X.XE_BIAS_M_RES),
    "k7d1-split": dict(kind="conv", ci=64, Kw=7, dil=1, hist=True, emode=X.XE_BIAS_M_RES, split=True),
    "tconv4s2": dict(kind="tconv", ci=32, Kw=4, stride=2, hist=True, emode=X.XE_BIAS_M),
    "tconv16s8-snake": dict(kind="tconv", ci=32, Kw=16, stride=8, hist=True, snake=True, emode=X.XE_BIAS_M),
}
SEG_CASES = [(b, nseg, N) for b in BASES for nseg in (1, 2, 5) for N in (1, 3, 64, 130)]


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.array(a)).to(gpu)      # (a copy: the shared reference inputs are read-only)


def _segment_inputs(sp, nseg):
    """shared weights and parameters (segment 0's), each segment its own input
    (and its own C before the call); per segment (d, ref, bound)"""
    d0 = X.reference(sp)[0]
    segs = []
    for s in range(nseg):
        ds = dict(d0)
        if s:
            own = X.make_inputs(replace(sp, seed=100 + s))
            ds["x"] = own["x"]
            if "c0" in own:
                ds["c0"] = own["c0"]
        acc, b_acc = X.accumulate(sp, ds)
        ref, bound = X.epilogue(sp, ds, acc, b_acc)
        segs.append((ds, ref, bound))
    return d0, segs


def _run_seg(gpu, sp, nseg, segs, d0, force, single=False):
    """one launch over the segments; (ran, C after [nseg, crows, ldc], C before)"""
    import torch
    lo = layout(sp)
    nan = np.float32(np.nan)
    keep, ptr = [], {}

    def put(name, a, off=0):
        t = _dev(np.asarray(a, np.float32), gpu)
        keep.append(t)
        ptr[name] = t.data_ptr() + 4 * off

    xs = np.stack([segs[s][0]["x"] for s in range(nseg)]).astype(np.float32)     # [nseg, ci, LM + N + RM]
    xs[:, :, :X.LM + sp.tmin] = nan                # left of the history: NaN, so a read into a neighbour shows
    xs[:, :, X.LM + sp.N:] = nan
    put("A", d0["w"])
    put("B", xs, X.LM)
    for k in ("sa", "sb", "bias", "ea", "eb"):
        if k in d0:
            put(k, d0[k])
    C0 = np.full((nseg, lo["crows"], lo["ldc"]), X.SENTINEL, np.float32)
    for s in range(nseg):
        if "c0" in segs[s][0]:
            c0 = segs[s][0]["c0"]
            C0[s, :c0.shape[0], :c0.shape[1]] = c0
    put("C", C0)
    desc = describe(sp, ptr)
    if single:
        ran = qtts.Kernels.xgemm_case(desc, sp.part, force)
    else:
        ran = qtts.Kernels.xgemm_seg_case(desc, nseg, sp.ci * lo["ldb"], lo["crows"] * lo["ldc"], sp.part, force)
    torch.cuda.synchronize()
    return ran, keep[-1].cpu().numpy(), C0


@pytest.mark.parametrize("base,nseg,N", SEG_CASES, ids=[f"{b}-seg{s}-N{n}" for b, s, n in SEG_CASES])
def test_segmented_conv(gpu, base, nseg, N):
    kw = dict(BASES[base])
    kind, split_ws = kw.pop("kind"), kw.pop("split", False)
    sp = X.Spec(kind, M_ROWS, N, **kw)
    if split_ws:       # a workspace that lets every segment keep two channel splits
        sp = replace(sp, part=2 * nseg * M_ROWS * sp.ncol)
    d0, segs = _segment_inputs(sp, nseg)
    ran_paths = []
    for force in (X.XP_CONVB2, X.XP_CONVB4, X.XP_CONV, X.XP_XGEMM, -1):
        ran, Cg, C0 = _run_seg(gpu, sp, nseg, segs, d0, force)
        if ran is None:                        # that kernel does not cover the shape: nothing ran
            assert force >= 0
            assert np.array_equal(Cg.view(np.uint32), C0.view(np.uint32))
            continue
        ran_paths.append(ran[0])
        assert force < 0 or ran[0] == force
        if nseg == 1:                          # the single-segment entry's plan, and its output bit for bit
            ran1, C1, _ = _run_seg(gpu, sp, 1, segs, d0, force, single=True)
            assert ran1 == ran, (ran1, ran)
            assert np.array_equal(C1.view(np.uint32), Cg.view(np.uint32))
        R, Cn = segs[0][1].shape
        worst = 0.0
        for s in range(nseg):
            ref, bound = segs[s][1], segs[s][2]
            got = Cg[s, :R, :Cn].astype(np.float64)
            assert np.all(np.isfinite(got)), (base, nseg, N, force, s)
            err = np.abs(got - ref)
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (base, nseg, N, force, s, worst, np.argwhere(~(err <= bound))[:4])
        mask = np.ones(Cg.shape, bool)
        mask[:, :R, :Cn] = False               # between and beside the segments: untouched, bit for bit
        assert np.array_equal(Cg.view(np.uint32)[mask], C0.view(np.uint32)[mask]), (base, nseg, N, force)
        print(f"err / bound  seg {base} nseg={nseg} N={N} {qtts.XP_NAMES[ran[0]]} x{ran[1]}: {worst:.4f}")
    # the generic kernel takes every conv form; the conv kernels take these channel counts
    assert X.XP_XGEMM in ran_paths and X.XP_CONVB2 in ran_paths and X.XP_CONV in ran_paths, ran_paths
