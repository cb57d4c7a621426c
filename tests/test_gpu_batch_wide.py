"""Lock-step decode of 17..64 slots: the wide batch GEMV (k_gemvx, through
qtts_hip_batch_matvec_case) against float64, its row independence bit for
bit, its split-K tickets, the same float64 bar under the 2..16-row kernels
(k_gemvb and k_gemvm), and the model on 17..64 slots against the oracle's
single runs (lock step, EOS queue with tail compaction across 16 rows, bf16
KV, teacher forcing, the 64-slot limit, one weight pass per GEMV).

Kernel bar (tests/test_gpu_kernels.py): |err| <= 2e-6 * (|W| @ |x|) + 1e-6 per
accumulated element, + 1e-5 * |ref| with the RMSNorm prologue; SwiGLU outputs
carry both halves' bounds through the product as test_resident_matvec does.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import manifest, model_dir
from oracle_py import DEFAULT, GREEDY, Oracle
from qtts_io import f32_to_bf16, lookup_ids
from synth_model import PRESETS, prompt_ids
from test_gpu_kernels import T, bf16_f64, gemv_bound
from test_gpu_model import audio_close

import qtts

pytestmark = pytest.mark.gpu

STORE, BIAS, BIAS_SILU, RESID, SWIGLU = range(5)
EPS = 1e-6


@functools.lru_cache(maxsize=4)
def _weights(R, Cc):
    rng = np.random.default_rng(R * 31 + Cc)
    return f32_to_bf16((rng.standard_normal((R, Cc)) / np.sqrt(Cc)).astype(np.float32))


def _epilogue(acc, bound, epi, y0, bias):
    """reference output and bound after the epilogue, from the accumulated [B, R]"""
    if epi == STORE:
        return acc, bound
    if epi == BIAS:
        return acc + bias, bound + 2e-7 * np.abs(acc + bias)
    if epi == BIAS_SILU:
        z = acc + bias
        return z / (1 + np.exp(-z)), 1.1 * bound + 1e-6 * (np.abs(z) + 1)
    if epi == RESID:
        return y0 + acc, bound + 2e-7 * (np.abs(y0) + np.abs(acc))
    B = acc.shape[0]
    q, qb = acc.reshape(B, -1, 2, 4), bound.reshape(B, -1, 2, 4)
    g, u = q[:, :, 0, :].reshape(B, -1), q[:, :, 1, :].reshape(B, -1)
    bsum = qb[:, :, 0, :].reshape(B, -1) + qb[:, :, 1, :].reshape(B, -1)
    return g / (1 + np.exp(-g)) * u, bsum * (np.abs(u) + np.abs(g) + 1)


def run_case(dev, R, Cc, B, *, norm=False, epi=STORE, src="x", n_part=0, xcopy=None, kz=0, self_reduce=True,
             row_sel=False, seed=0, x_override=None, kernel=None, A_override=None):
    """One qtts_hip_batch_matvec_case against float64.  Returns (got, ref,
    bound) of y (or of the summed consumer-add partials), after asserting the
    xcopy output.  Inputs and partials are of order 1, so a dropped partial or
    row is far outside the bound.  kernel: the kernel the planner must have
    chosen for the case (qtts_hip_batch_matvec_plan on the same arguments).
    A_override: the weights' bf16 bits in place of the random ones."""
    import torch
    rng = np.random.default_rng(seed + R + 3 * Cc + 7 * B)
    A = _weights(R, Cc) if A_override is None else A_override
    w = (1 + 0.1 * rng.standard_normal(Cc)).astype(np.float32) if norm else None
    kw = {}
    if src == "x":
        x = (rng.standard_normal((B, Cc)) * 2).astype(np.float32) if x_override is None else x_override
        xin = x.astype(np.float64)
        kw["x"] = T(x, dev)
        if n_part:
            part = rng.standard_normal((n_part, B, Cc)).astype(np.float32)
            ps = part[0].astype(np.float32)
            for p in range(1, n_part):   # (p0 + p1 + ...) in fp32, in order, as the kernel adds them
                ps = ps + part[p]
            xin = (x + ps).astype(np.float64)   # fp32 sum, as the kernel forms it
            kw["part_in"] = T(part, dev)
    else:
        nrows_t, sel_n = 200, 3
        tab = (rng.standard_normal((nrows_t, Cc)) * 2).astype(np.float32)
        ids = rng.integers(0, nrows_t, size=(B, sel_n + 2)).astype(np.int32)   # [b][ids_off + row_sel * rstride]
        sel = rng.integers(0, sel_n, size=B).astype(np.int32) if row_sel else None
        off = 1
        pick = ids[np.arange(B), off + (sel if row_sel else 0)]
        if src == "tab16":
            t16 = f32_to_bf16(tab)
            xin = bf16_f64(t16)[pick]
            kw["table"] = T(t16, dev, torch.int16)
        else:
            xin = tab[pick].astype(np.float64)
            kw["table"] = T(tab, dev)
        kw.update(ids_i32=T(ids, dev), ids_bstride=sel_n + 2, ids_rstride=1, ids_off=off,
                  row_sel_i32=T(sel, dev) if row_sel else None)
    xn = xin
    if norm:
        xn = xin / np.sqrt((xin ** 2).mean(1, keepdims=True) + EPS) * w
        kw["norm_w"] = T(w, dev)
    Af = bf16_f64(A)
    acc = xn @ Af.T
    bound = gemv_bound(A, xn) + (1e-5 * np.abs(acc) if norm else 0)
    nout = R // 2 if epi == SWIGLU else R
    y0 = rng.standard_normal((B, nout)).astype(np.float32) if epi == RESID else np.zeros((B, nout), np.float32)
    bias = rng.standard_normal(R).astype(np.float32) if epi in (BIAS, BIAS_SILU) else None
    y = T(y0.copy(), dev)
    xc = torch.full((B, Cc), float("nan"), device=dev) if xcopy else None
    part_out = None
    if kz and not self_reduce:
        part_out = torch.full((kz, B, R), float("nan"), device=dev)
    kw.update(eps=EPS, xcopy=xc, xcopy_normed=xcopy == "normed", epi=epi,
              bias=T(bias, dev) if bias is not None else None, kz=kz, self_reduce=self_reduce, part_out=part_out)
    Ad = T(A, dev, torch.int16)
    if kernel is not None:
        plan = qtts.Kernels.batch_matvec_plan(qtts.Kernels.bgemv_desc(Ad, B, y, **kw))
        assert plan is not None, "no batch kernel covers the case"
        assert plan["kernel"] == kernel, plan
    ok = qtts.Kernels.batch_matvec_case(Ad, B, y, **kw)
    assert ok, "no batch kernel covers the case"
    torch.cuda.synchronize()
    if xcopy:
        want = xn if xcopy == "normed" else xin
        tol = 1e-5 * np.abs(want) + 1e-6 if xcopy == "normed" else 0.0
        assert np.all(np.abs(xc.cpu().numpy() - want) <= tol), np.abs(xc.cpu().numpy() - want).max()
    if part_out is not None:
        p = part_out.cpu().numpy().astype(np.float64)
        return y0 + p.sum(0), y0 + acc, bound + 2e-7 * (np.abs(y0) + np.abs(acc)) + 2e-7 * np.abs(p).sum(0)
    ref, bound = _epilogue(acc, bound, epi, y0, bias)
    return y.cpu().numpy(), ref, bound


def check(got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(np.isfinite(got)) and np.all(err <= bound), float(np.max(err / bound))


# ---------------------------------------------------------------- 1. kernel bar
BATCHES = [17, 31, 32, 33, 48, 63, 64]
SMALL = [(128, 64), (256, 128), (48, 96), (1040, 192)]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("R,Cc", SMALL)
def test_wide_small_shapes(gpu, R, Cc, B):
    """every batch size at the smallest shapes that can go wrong: the tiny
    presets', one ragged weight-tile group with 3 K steps, a 65-tile 6-step
    one; plain, normed with both copies, residual, and bias + SiLU"""
    check(*run_case(gpu, R, Cc, B))
    check(*run_case(gpu, R, Cc, B, norm=True, xcopy="normed"))
    check(*run_case(gpu, R, Cc, B, epi=RESID, xcopy="raw"))
    check(*run_case(gpu, R, Cc, B, norm=True, epi=BIAS_SILU))
    check(*run_case(gpu, R, Cc, B, epi=BIAS))


@pytest.mark.parametrize("B", [17, 40, 64])
@pytest.mark.parametrize("src,row_sel", [("tab16", False), ("tab16", True), ("tabf", True)])
def test_wide_table_sources(gpu, B, src, row_sel):
    """bf16 and fp32 table rows gathered by id (with and without the row
    selector), normed, raw copy written"""
    check(*run_case(gpu, 256, 128, B, norm=True, src=src, row_sel=row_sel, xcopy="raw"))
    check(*run_case(gpu, 256, 128, B, norm=True, epi=SWIGLU, src=src, row_sel=row_sel))


@pytest.mark.parametrize("B", [17, 33, 64])
def test_wide_small_split_k_and_partials(gpu, B):
    """partials in (1..4), split-K out self-reducing and consumer-add, at a small shape"""
    for n in (1, 2, 3, 4):
        check(*run_case(gpu, 256, 128, B, norm=True, epi=SWIGLU, n_part=n, xcopy="raw"))
    for kz in (2, 4):
        check(*run_case(gpu, 256, 128, B, epi=RESID, kz=kz, self_reduce=True))
        check(*run_case(gpu, 256, 128, B, epi=RESID, kz=kz, self_reduce=False))


REAL = [
    ("qkv", 4096, 2048, dict(norm=True)),
    ("gate_up", 12288, 2048, dict(norm=True, epi=SWIGLU)),
    ("o_kz2_self", 2048, 2048, dict(epi=RESID, kz=2)),
    ("o_kz4_self", 2048, 2048, dict(epi=RESID, kz=4)),
    ("o_kz2_cons", 2048, 2048, dict(epi=RESID, kz=2, self_reduce=False)),
    ("o_kz4_cons", 2048, 2048, dict(epi=RESID, kz=4, self_reduce=False)),
    ("down_kz4", 2048, 6144, dict(epi=RESID, kz=4)),
    ("head", 3072, 2048, dict(norm=True, xcopy="normed")),
    ("st_qkv_tabf", 4096, 1024, dict(src="tabf", row_sel=True)),
    ("st_gate_up_p2", 6144, 1024, dict(norm=True, epi=SWIGLU, n_part=2)),
    ("st_gate_up_p4", 6144, 1024, dict(norm=True, epi=SWIGLU, n_part=4)),
    ("st_down", 1024, 3072, dict(epi=RESID)),
    ("st_lm", 2048, 1024, dict(norm=True)),
]


@pytest.mark.parametrize("B", [24, 64])
@pytest.mark.parametrize("name,R,Cc,kw", REAL, ids=[r[0] for r in REAL])
def test_wide_real_shapes(gpu, name, R, Cc, kw, B):
    """the 1.7B talker's and sub-talker's decode GEMVs, once each at 24 and 64 rows"""
    check(*run_case(gpu, R, Cc, B, **kw))


# ---------------------------------------------------------------- 1b. the same bar under the 2..16-row kernels
NARROW = [2, 7, 8, 9, 16]
NARROW_KERNELS = [("k_gemvb", None), ("k_gemvm", "0")]   # (kernel planned, QTTS_HIP_GEMVB)


@pytest.fixture(params=NARROW_KERNELS, ids=[k for k, _ in NARROW_KERNELS])
def narrow_kernel(request, monkeypatch):
    """the planner's default at 2..16 rows (k_gemvb takes every case below),
    then k_gemvm through QTTS_HIP_GEMVB=0; run_case asserts the plan"""
    kernel, env = request.param
    if env is None:
        monkeypatch.delenv("QTTS_HIP_GEMVB", raising=False)
    else:
        monkeypatch.setenv("QTTS_HIP_GEMVB", env)
    monkeypatch.delenv("QTTS_HIP_GB_W", raising=False)
    return kernel


@pytest.mark.parametrize("B", NARROW)
@pytest.mark.parametrize("R,Cc", SMALL)
def test_narrow_small_shapes(gpu, narrow_kernel, R, Cc, B):
    """the five forms of test_wide_small_shapes at 2..16 rows, on k_gemvb and on k_gemvm"""
    k = narrow_kernel
    check(*run_case(gpu, R, Cc, B, kernel=k))
    check(*run_case(gpu, R, Cc, B, norm=True, xcopy="normed", kernel=k))
    check(*run_case(gpu, R, Cc, B, epi=RESID, xcopy="raw", kernel=k))
    check(*run_case(gpu, R, Cc, B, norm=True, epi=BIAS_SILU, kernel=k))
    check(*run_case(gpu, R, Cc, B, epi=BIAS, kernel=k))


@pytest.mark.parametrize("B", NARROW)
@pytest.mark.parametrize("src,row_sel", [("tab16", False), ("tab16", True), ("tabf", True)])
def test_narrow_table_sources(gpu, narrow_kernel, B, src, row_sel):
    """the forms of test_wide_table_sources at 2..16 rows, on k_gemvb and on k_gemvm"""
    k = narrow_kernel
    check(*run_case(gpu, 256, 128, B, norm=True, src=src, row_sel=row_sel, xcopy="raw", kernel=k))
    check(*run_case(gpu, 256, 128, B, norm=True, epi=SWIGLU, src=src, row_sel=row_sel, kernel=k))


@pytest.mark.parametrize("B", NARROW)
def test_narrow_small_split_k_and_partials(gpu, narrow_kernel, B):
    """the forms of test_wide_small_split_k_and_partials at 2..16 rows, on k_gemvb and on k_gemvm"""
    k = narrow_kernel
    for n in (1, 2, 3, 4):
        check(*run_case(gpu, 256, 128, B, norm=True, epi=SWIGLU, n_part=n, xcopy="raw", kernel=k))
    for kz in (2, 4):
        check(*run_case(gpu, 256, 128, B, epi=RESID, kz=kz, self_reduce=True, kernel=k))
        check(*run_case(gpu, 256, 128, B, epi=RESID, kz=kz, self_reduce=False, kernel=k))


# ---------------------------------------------------------------- 1c. exact planes
# The 2e-6 bound above cannot see a lost third bf16 plane of x (at most 0.21 of
# the bound on these inputs' kind; rows_gemm_ref.py).  The three batch kernels
# split x into three planes as the multi-row GEMMs do, so they run the same
# instrument: inputs whose planes are known and whose every partial sum is
# exact in fp32 (rows_gemm_ref.exact_inputs), so the result equals the float64
# one bit for bit whatever the order, K slot or split column.
EXACT_SHAPE = (256, 128)   # the smallest shape of SMALL all three planners take with and without kz
EXACT_RUNS = [("k_gemvb", None, 2), ("k_gemvb", None, 16), ("k_gemvm", "0", 2), ("k_gemvm", "0", 16),
              ("k_gemvx", None, 17), ("k_gemvx", None, 64)]


@pytest.mark.parametrize("kernel,env,B", EXACT_RUNS, ids=[f"{k}-{B}" for k, _, B in EXACT_RUNS])
def test_exact_planes_bit_equal_float64(gpu, monkeypatch, kernel, env, B):
    """store without kz, and kz 2 both consumer-add (the raw partials summed in
    float64 here) and self-reducing (y0 + (p0 + p1): one fp32 rounding of the
    exact float64 sum)"""
    from rows_gemm_ref import exact_inputs
    if env is None:
        monkeypatch.delenv("QTTS_HIP_GEMVB", raising=False)
    else:
        monkeypatch.setenv("QTTS_HIP_GEMVB", env)
    monkeypatch.delenv("QTTS_HIP_GB_W", raising=False)
    R, Cc = EXACT_SHAPE
    A, x, _ = exact_inputs(B, R, Cc, np.random.default_rng(1000 + B))
    kw = dict(x_override=x, A_override=A, kernel=kernel)
    got, ref, _ = run_case(gpu, R, Cc, B, **kw)
    assert np.array_equal(got.astype(np.float64), ref), int(np.count_nonzero(got.astype(np.float64) != ref))
    got, ref, _ = run_case(gpu, R, Cc, B, epi=RESID, kz=2, self_reduce=False, **kw)
    assert np.array_equal(got, ref), int(np.count_nonzero(got != ref))
    got, ref, _ = run_case(gpu, R, Cc, B, epi=RESID, kz=2, self_reduce=True, **kw)
    assert got.dtype == np.float32
    assert np.array_equal(got, ref.astype(np.float32)), int(np.count_nonzero(got != ref.astype(np.float32)))


# ---------------------------------------------------------------- 2. row independence, bitwise
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("epi", [STORE, SWIGLU])
def test_wide_rows_independent_bitwise(gpu, norm, epi):
    """batch 40, (256, 128): permuted rows give the permuted output exactly;
    one row at positions 0, 15, 16, 33, 39 gives five identical output rows,
    and they do not move when every other row changes"""
    R, Cc, B = 256, 128, 40
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((B, Cc)) * 2).astype(np.float32)
    same = [0, 15, 16, 33, 39]
    x[same] = x[0]
    y, ref, bound = run_case(gpu, R, Cc, B, norm=norm, epi=epi, x_override=x)
    check(y, ref, bound)
    for i in same[1:]:
        np.testing.assert_array_equal(y[i], y[0])
    perm = rng.permutation(B)
    yp, _, _ = run_case(gpu, R, Cc, B, norm=norm, epi=epi, x_override=np.ascontiguousarray(x[perm]))
    np.testing.assert_array_equal(yp, y[perm])
    x2 = (rng.standard_normal((B, Cc)) * 5).astype(np.float32)
    x2[same] = x[0]
    y2, _, _ = run_case(gpu, R, Cc, B, norm=norm, epi=epi, x_override=x2)
    for i in same:
        np.testing.assert_array_equal(y2[i], y[0])


# ---------------------------------------------------------------- 3. tickets reset
@pytest.mark.parametrize("B,R,Cc,kz", [(40, 256, 128, 4), (24, 2048, 2048, 2)])
def test_wide_tickets_reset(gpu, B, R, Cc, kz):
    """the same self-reducing case twice on one stream (the library keeps the
    tickets between calls): equal results, so no ticket was left counting"""
    a = run_case(gpu, R, Cc, B, epi=RESID, kz=kz, self_reduce=True)
    b = run_case(gpu, R, Cc, B, epi=RESID, kz=kz, self_reduce=True)
    check(*a)
    np.testing.assert_array_equal(a[0], b[0])


# ---------------------------------------------------------------- 4. model, tiny presets vs the oracle port
SPK = ["aiden", "vivian", "serena"]
LANG = ["english", "japanese", "chinese", "english"]
_ORC = {}


def _prompt(i):
    return prompt_ids("short") if i % 7 == 0 else prompt_ids("p128", 2000 + i)


def _oracle_single(o, tag, i, pp_name, fixed, max_tokens=4096, seed=42):
    """the oracle's single run of utterance i (codes, stop reason, waveform), once per session"""
    key = (tag, i, pp_name, fixed, max_tokens, seed)
    if key not in _ORC:
        s, l = lookup_ids(o.cfg, SPK[i % 3], LANG[i % 4])
        pp = GREEDY if pp_name == "greedy" else DEFAULT
        codes, stop = o.generate_codes(_prompt(i), s, l, max_tokens=max_tokens, fixed=fixed, seed=seed, **pp)
        _ORC[key] = (codes, stop, o.codec_decode(codes))
    return _ORC[key]


def _lock_step(m, o, tag, nb):
    prompts = [_prompt(i) for i in range(nb)]
    spk, lang = [SPK[i % 3] for i in range(nb)], [LANG[i % 4] for i in range(nb)]
    w0 = qtts.Kernels.gemv_wide_launches()
    for pp_name, pp in (("greedy", GREEDY), ("default", DEFAULT)):
        m.set_params(max_tokens=4096, fixed=8, seed=42, **pp)
        rc, audio = m.generate_batch(prompts, spk, lang)
        assert rc == 0
        for b in range(nb):
            audio_close(audio[b], _oracle_single(o, tag, b, pp_name, 8)[2])
        rc, again = m.generate_batch(prompts, spk, lang)
        assert rc == 0
        for b in range(nb):
            np.testing.assert_array_equal(again[b], audio[b])
    assert qtts.Kernels.gemv_wide_launches() > w0   # (the wide kernel ran, not a per-16-row fallback)


@pytest.mark.parametrize("nb", [17, 33, 64])
def test_lock_step_slots_match_single_runs(tiny_dir, oracle, nb):
    """17 / 33 / 64 lock-step slots, mixed prompts, speakers and languages,
    greedy and default sampling, 8 frames: every slot's audio equals the
    oracle's decode of its own single run; a second call is bit-identical"""
    m = qtts.QwenTTS(tiny_dir)
    try:
        _lock_step(m, oracle, "tiny", nb)
    finally:
        m.close()


def test_lock_step_33_slots_tiny_eq(tiny_eq_dir):
    """the same on the preset without the sub-talker input projection (bf16 table rows by id)"""
    o = Oracle(tiny_eq_dir)
    m = qtts.QwenTTS(tiny_eq_dir)
    try:
        _lock_step(m, o, "tiny_eq", 33)
    finally:
        m.close()
        o.close()


def test_eos_queue_60_on_20_slots(gpu):
    """EOS mode, 60 utterances on 20 slots with tail compaction: every
    utterance's codes and stop reason equal its oracle single run, and the
    frames were launched on row counts both above and below 16 (the tail walks
    down from the wide kernel to the 16-row ones).  The per-frame row counts
    are rebuilt from the progress callback (done count after every frame: once
    nothing is left to admit the next frame runs the remaining utterances) and
    must add up to queue_rows_launched exactly."""
    md = model_dir("tiny", eos_gain=manifest()["eos_gain"])
    o, m = Oracle(md), qtts.QwenTTS(md)
    nq, ns = 60, 20
    done = []
    cb = qtts.PROGRESS_CB(lambda s, t, u: done.append(s))
    qtts.lib().qwen_tts_set_progress_callback(m.ctx, cb, None)
    try:
        # the first 60 utterances whose oracle run has a frame at all (one that
        # draws EOS at once has no audio, and the queue call reports that as -1)
        utt, i = [], 0
        while len(utt) < nq:
            if len(_oracle_single(o, "tiny_eos", i, "default", 0, max_tokens=32, seed=7)[0]) > 0:
                utt.append(i)
            i += 1
        prompts = [_prompt(i) for i in utt]
        m.set_params(max_tokens=32, fixed=0, seed=7, **DEFAULT)
        rc, audio = m.generate_queue(prompts, [SPK[i % 3] for i in utt], [LANG[i % 4] for i in utt], slots=ns)
        assert rc == 0
        st = m.queue_stats()
        assert st["slots"] == ns and st["refills"] == nq - ns, st
        for k, i in enumerate(utt):
            want, stop, _ = _oracle_single(o, "tiny_eos", i, "default", 0, max_tokens=32, seed=7)
            np.testing.assert_array_equal(m.queue_codes(k), want, err_msg=f"utterance {k} (prompt {i})")
            assert st["stop_reason"][k] == stop, (k, st["stop_reason"][k], stop)
        # frames 0 and 1 run every slot; the callback after frame s >= 1 fixes frame s + 1's rows
        rows = [ns, ns]
        for d in done[:st["frames"] - 2]:
            rows.append(min(rows[-1], nq - d) if d > nq - ns else rows[-1])
        assert len(rows) == st["frames"] and sum(rows) == st["rows_launched"], (rows, st)
        assert max(rows) > 16 and min(rows) <= 16 and any(16 < r < ns for r in rows), rows
    finally:
        qtts.lib().qwen_tts_set_progress_callback(m.ctx, C.cast(None, qtts.PROGRESS_CB), None)
        m.close()
        o.close()


def test_bf16_kv_20_slots_equal_single_runs(tiny_dir):
    """bf16 KV, 20 slots: every slot's codes equal the same utterance's bf16-KV
    single run (the mode's own self-consistency bar, not the reference's)"""
    m = qtts.QwenTTS(tiny_dir)
    try:
        m.set_kv_cache("bf16")
        nb = 20
        prompts = [_prompt(i) for i in range(nb)]
        m.set_params(max_tokens=64, fixed=8, seed=11, **DEFAULT)
        single = []
        for i in range(nb):
            assert m.generate(prompts[i], SPK[i % 3], LANG[i % 4]) is not None
            single.append(m.last_codes())
        rc, _ = m.generate_batch(prompts, [SPK[i % 3] for i in range(nb)], [LANG[i % 4] for i in range(nb)])
        assert rc == 0 and m.kv_cache() == qtts.KV_BF16
        for b in range(nb):
            np.testing.assert_array_equal(m.last_codes_slot(b, 64), single[b], err_msg=f"batch row {b}")
    finally:
        m.close()


def test_forced_prefix_on_slot_18_of_20(tiny_dir):
    """teacher forcing at 20 slots: slot 18 forced onto a prefix of its own
    codes -- the other 19 slots' codes and audio unchanged, slot 18's free-draw
    record (and codes) equal to its plain run"""
    m = qtts.QwenTTS(tiny_dir)
    try:
        nb = 20
        prompts = [_prompt(i) for i in range(nb)]
        spk, lang = [SPK[i % 3] for i in range(nb)], [LANG[i % 4] for i in range(nb)]
        m.set_params(max_tokens=4096, fixed=8, seed=42, **DEFAULT)
        rc, a0 = m.generate_batch(prompts, spk, lang)
        assert rc == 0
        c0 = m.last_codes_batch(nb, 8)
        m.force_codes(c0[18][:5].copy(), slot=18)
        rc, a1 = m.generate_batch(prompts, spk, lang)
        assert rc == 0
        c1 = m.last_codes_batch(nb, 8)
        for b in range(nb):
            np.testing.assert_array_equal(c1[b], c0[b], err_msg=f"slot {b}")
            np.testing.assert_array_equal(a1[b], a0[b], err_msg=f"slot {b}")
        np.testing.assert_array_equal(m.last_drawn(18), c0[18])
    finally:
        m.close()


def test_65_slots_refused_and_context_usable(tiny_dir):
    """65 slots: -1 from generate_batch and from generate_queue; the next 4-slot call succeeds"""
    m = qtts.QwenTTS(tiny_dir)
    try:
        m.set_params(max_tokens=4096, fixed=4, seed=42, **GREEDY)
        p65 = [prompt_ids("short")] * 65
        rc, audio = m.generate_batch(p65, ["aiden"] * 65, ["english"] * 65)
        assert rc == -1 and all(a is None for a in audio)
        rc, audio = m.generate_queue(p65, ["aiden"] * 65, ["english"] * 65, slots=65)
        assert rc == -1 and all(a is None for a in audio)
        rc, audio = m.generate_batch(p65[:4], ["aiden"] * 4, ["english"] * 4)
        assert rc == 0 and all(a is not None and len(a) == 4 * 1920 for a in audio)
    finally:
        m.close()


# ---------------------------------------------------------------- 5. one weight pass per GEMV
def _gemvs_per_frame(preset):
    """decode GEMV launches of a lock-step frame (>= 2 slots), from the layer
    counts: (first frame, later frames).  Talker: q|k|v, O, gate|up, down per
    layer + the codec head (the first frame starts from the prefill's hidden:
    head only).  Sub-talker pass 0: 4 per layer but its last, which only
    stores k / v (q|k|v alone), no head, + the input projection of the talker
    hidden where H != Hs; passes 1..G-1: their input projection is a gather
    from the load-time table (no launch), layer 0 reads its q|k|v from the
    load-time table too (NHs == 2 KVs: no GEMV), so 4 Ls - 1, + the lm head."""
    p = PRESETS[preset]
    assert p["NHs"] == 2 * p["KVs"]
    proj0 = 1 if p["H"] != p["Hs"] else 0
    sub = proj0 + 4 * (p["Ls"] - 1) + 1 + (p["G"] - 1) * (4 * p["Ls"] - 1 + 1)
    return 1 + sub, 4 * p["L"] + 1 + sub


def test_one_wide_launch_per_gemv(tiny_dir, monkeypatch):
    """an 8-frame run launches the same number of wide GEMVs at 17, 32 and 64
    slots -- frames x the per-frame GEMV count, one launch (one weight read)
    each -- and none at 16 slots.  Launch-per-op frames (QTTS_HIP_NO_GRAPH):
    a captured graph would count its launches once, not per frame."""
    monkeypatch.setenv("QTTS_HIP_NO_GRAPH", "1")
    m = qtts.QwenTTS(tiny_dir)
    try:
        first, later = _gemvs_per_frame("tiny")
        m.set_params(max_tokens=4096, fixed=8, seed=42, **GREEDY)
        grew = {}
        for nb in (16, 17, 32, 64):
            w0 = qtts.Kernels.gemv_wide_launches()
            rc, _ = m.generate_batch([_prompt(i) for i in range(nb)], ["aiden"] * nb, ["english"] * nb)
            assert rc == 0
            grew[nb] = qtts.Kernels.gemv_wide_launches() - w0
        assert grew[16] == 0, grew
        assert grew[17] == grew[32] == grew[64] == first + 7 * later, (grew, first, later)
    finally:
        m.close()


# ---------------------------------------------------------------- 6. full size, against the reference's own runs
def _b8():
    import json
    import os
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "long_17b_b8.npz"))
    man = json.load(open(os.path.join(GOLDEN, "long_manifest.json")))["b8"]
    prompts = [g["prompt_ids"][b, :int(g["prompt_len"][b])] for b in range(g["prompt_ids"].shape[0])]
    return g, man, prompts


@pytest.mark.slow
@pytest.mark.parametrize("nb,frames", [(24, 32), (40, 32), (64, 8)])
def test_17b_wide_lock_step_vs_reference(gpu, nb, frames):
    """The 8 reference utterances of long_17b_b8.npz (three speakers, default
    sampling) repeated to 24 / 40 / 64 lock-step slots, rotated by one per
    repetition so the replicas of an utterance sit at different rows of
    different 16-row groups: every slot's codes bit-exact against its
    reference run (32 frames; the 64-slot run decodes 8 frames against the
    reference's first 8), replicas bit-identical in codes and audio, last-frame
    audio against the reference's at 32 frames.  A differing draw is a finding
    (tests/parity.py names its frame and group), not a tolerance."""
    from parity import codes_equal
    from test_gpu_long import _audio_close
    g, man, prompts = _b8()
    utt = [(s + s // 8) % 8 for s in range(nb)]
    m = qtts.QwenTTS(model_dir("1.7b"))
    try:
        w0 = qtts.Kernels.gemv_wide_launches()
        m.set_params(max_tokens=4096, fixed=frames, seed=man["seed"], **DEFAULT)
        rc, audio = m.generate_batch([prompts[u] for u in utt], [man["speakers"][u] for u in utt],
                                     [man["language"]] * nb)
        assert rc == 0 and qtts.Kernels.gemv_wide_launches() > w0
        codes = m.last_codes_batch(nb, frames)
        first = {}
        for s, u in enumerate(utt):
            codes_equal(codes[s], g["codes"][u][:frames], f"batch-{nb} slot {s} (utterance {u})")
            if frames == man["frames"]:
                _audio_close(audio[s][-1920:], g["audio_last"][u], f"slot {s} last frame")
            if u in first:
                np.testing.assert_array_equal(codes[s], codes[first[u]])
                np.testing.assert_array_equal(audio[s], audio[first[u]])
            first.setdefault(u, s)
    finally:
        m.close()
