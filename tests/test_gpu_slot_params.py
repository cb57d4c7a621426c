"""Per-utterance sampling parameters and seeds in batch and queue decode
(`qwen_tts_set_utterance_sampling`, `qtts_dev_slot_params`, the per-slot
sampler k_sample_p.hip).

The bar is the one batch and queue already meet: every utterance decodes bit
for bit as it would alone with its own parameters and seed -- the reference
decodes one utterance per call with the ctx's parameters (Q.c:1059-1443) --
whatever slot it lands in and whatever the other slots draw.

1. the per-slot sampler kernels row by row against the oracle's orc_sample
   (ids and RNG states bit-exact), both families and QTTS_HIP_SAMPLE_W=0;
2. a 12-slot batch over six parameter sets x two seeds against the oracle's
   single runs (EOS mode, three prompts, fixed mode);
3. an armed run with the ctx's own values equals the unarmed one, the next run
   is plain again, and the launch counter says which sampler ran;
4. 20 slots (the wide batch kernel);
5. the work queue: rows follow their utterances through refills and the tail
   compaction, and the first full-path row arrives by refill;
6. refusals;  7. (slow) the synthetic 1.7B;  8. the CLI's --seed-step.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import manifest, model_dir
from oracle_py import DEFAULT, Oracle, fptr
from parity import codes_equal
from qtts_io import lookup_ids
from synth_model import prompt_ids

import qtts

pytestmark = pytest.mark.gpu

SETS = {
    "default": {},
    "hot": dict(temperature=1.4, top_k=0, st_temperature=1.3),
    "nucleus": dict(top_p=0.8, st_top_p=0.7),
    "greedy": dict(top_k=1, st_top_k=1),
    "rep15": dict(rep=1.5),
    "k300": dict(top_k=300, st_top_k=7, temperature=0.6),
}
# the sets whose two draws both take the fast path (top_p >= 1, 0 < top_k <= 1024)
FAST_SETS = ("default", "greedy", "rep15", "k300")


def _params(name):
    p = dict(DEFAULT)
    p.update(SETS[name])
    return p


def T(a, dev, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.view(dtype)
    return t.to(dev)


# ---------------------------------------------------------------- 1. the kernels
K_CHOICES, P_CHOICES = [1, 50, 0, 7, 300, 2048], [1.0, 0.9, 0.5, 0.99]


def _row_fast(k, tp, V):
    return tp >= 1.0 and 0 < k < V and k <= 1024


def _rows(rng, B, V, kind):
    """B (top_k, top_p, temperature) rows: all fast-path eligible, all needing
    the full path, or the two interleaved"""
    fast = [(k, 1.0) for k in K_CHOICES if _row_fast(k, 1.0, V)]
    full = [(k, tp) for k in K_CHOICES for tp in P_CHOICES if not _row_fast(k, tp, V)]
    rows = []
    for b in range(B):
        pool = fast if kind == "fast" or (kind == "mixed" and b % 2 == 0) else full
        k, tp = pool[int(rng.integers(0, len(pool)))]
        rows.append((k, tp, float(rng.uniform(0.4, 1.6))))
    return rows


def _logits(rng, B, V, it):
    """the logit patterns of test_sampler_random_vs_oracle and
    test_sampler_candidate_bins_vs_oracle: ties at the maximum, ties straddling
    the k-th key, -1e9 blocks, ineligible -FLT_MAX entries"""
    lg = (rng.standard_normal((B, V)) * rng.uniform(0.3, 8)).astype(np.float32)
    if it % 3 == 0:
        lg[:, rng.integers(0, V, 30)] = lg.max()
    if it % 5 == 1:
        lg[:, rng.integers(0, V, V // 3)] = -1e9
    if it % 4 == 2:
        for b in range(B):
            lg[b, rng.integers(0, V, min(80, V // 2))] = np.sort(lg[b])[::-1][min(45, V - 1)]
    if it % 7 == 3 and V > 40:
        lg[:, rng.integers(0, V, V - 20)] = -np.finfo(np.float32).max
    return lg


def _sample_rows(dev, lg, V, rows, st0):
    import torch
    B = lg.shape[0]
    out = torch.zeros(B, dtype=torch.int32, device=dev)
    rs = T(np.asarray(st0, np.float32).view(np.int32), dev)
    n0 = qtts.Kernels.sample_slot_launches()
    qtts.Kernels.sample_top_k_rows(out, T(lg, dev), V, [r[0] for r in rows], [r[1] for r in rows],
                                   [r[2] for r in rows], rs, B)
    torch.cuda.synchronize()
    assert qtts.Kernels.sample_slot_launches() == n0 + 1
    return out.cpu().numpy(), rs.cpu().numpy().view(np.uint32)


def _check_rows(oracle, lg, V, rows, st0, r, st, what):
    for b, (k, tp, temp) in enumerate(rows):
        s = np.array([st0[b]], np.float32)
        e = oracle.lib.orc_sample(fptr(lg[b].copy()), V, k, tp, temp, fptr(s))
        assert r[b] == e, (what, b, rows[b], int(r[b]), e)
        assert st[b] == s.view(np.uint32)[0], (what, b, rows[b])


@pytest.mark.parametrize("sw", ["1", "0"])
def test_per_row_sampler_vs_oracle(gpu, oracle, monkeypatch, sw):
    """every row of a launch draws with its own top_k / top_p / temperature:
    all-fast launches (the 1024-thread family, or the general kernel with
    QTTS_HIP_SAMPLE_W=0), all-full and mixed launches (the general kernel),
    V 64 .. 4096, 1 .. 17 rows; ids and RNG states bit-exact"""
    monkeypatch.setenv("QTTS_HIP_SAMPLE_W", sw)
    rng = np.random.default_rng(2024)
    it = 0
    for V in (64, 1500, 2048, 3072, 4096):
        for B in (1, 3, 8, 17):
            for kind in ("fast", "full", "mixed"):
                lg = _logits(rng, B, V, it)
                rows = _rows(rng, B, V, kind)
                st0 = rng.integers(1, 10**6, B).astype(np.float32)
                r, st = _sample_rows(gpu, lg, V, rows, st0)
                _check_rows(oracle, lg, V, rows, st0, r, st, (V, B, kind, it))
                it += 1


@pytest.mark.parametrize("sw", ["1", "0"])
@pytest.mark.parametrize("V", [2048, 3072])
def test_per_row_sampler_invariants(gpu, oracle, monkeypatch, sw, V):
    """identical logits and RNG state in every row, different parameters: each
    row equals its own orc_sample; the same parameters in every row: the result
    equals qtts_hip_sample_top_k on the same input, byte for byte"""
    import torch
    monkeypatch.setenv("QTTS_HIP_SAMPLE_W", sw)
    rng = np.random.default_rng(V)
    B = 8
    one = (rng.standard_normal(V) * 3.0).astype(np.float32)
    lg = np.tile(one, (B, 1))
    st0 = np.full(B, 4711.0, np.float32)
    for kind in ("fast", "mixed"):
        rows = _rows(rng, B, V, kind)
        r, st = _sample_rows(gpu, lg, V, rows, st0)
        _check_rows(oracle, lg, V, rows, st0, r, st, (V, kind, "identical logits"))
    lg = _logits(rng, B, V, 0)
    st0 = rng.integers(1, 10**6, B).astype(np.float32)
    for k, tp, temp in ((50, 1.0, 0.9), (300, 1.0, 0.7), (50, 0.9, 1.1), (0, 1.0, 1.3)):
        r, st = _sample_rows(gpu, lg, V, [(k, tp, temp)] * B, st0)
        out = torch.zeros(B, dtype=torch.int32, device=gpu)
        rs = T(st0.view(np.int32), gpu)
        qtts.Kernels.sample_top_k(out, T(lg, gpu), V, k, tp, temp, rs, B)
        torch.cuda.synchronize()
        assert r.tobytes() == out.cpu().numpy().tobytes(), (k, tp, temp)
        assert st.tobytes() == rs.cpu().numpy().view(np.uint32).tobytes(), (k, tp, temp)


# ---------------------------------------------------------------- 2. - 6. the tiny EOS model
@pytest.fixture(scope="module")
def tiny_eos(gpu):
    md = model_dir("tiny", eos_gain=manifest()["eos_gain"])
    m = qtts.QwenTTS(md)
    o = Oracle(md)
    yield m, o
    m.close()
    o.close()


_ORC = {}


def _single(o, ids, name, seed, max_tokens=32, fixed=0):
    """the oracle's single run of one utterance with its own parameter set and
    seed: (codes, stop reason 1 eos / 2 max_tokens, waveform), once per session"""
    key = (tuple(int(i) for i in ids), name, seed, max_tokens, fixed)
    if key not in _ORC:
        s, l = lookup_ids(o.cfg, "aiden", "english")
        codes, stop = o.generate_codes(ids, s, l, max_tokens=max_tokens, fixed=fixed, seed=seed, **_params(name))
        _ORC[key] = (codes, stop, o.codec_decode(codes))
    return _ORC[key]


def _audio_close(a, ref, what):
    assert a is not None and a.shape == ref.shape, (what, None if a is None else a.shape, ref.shape)
    d = a.astype(np.float64) - ref
    mse = float(np.mean(d * d))
    assert mse < 1e-4, (what, mse)


def _check_utt(o, got, audio, ids, name, seed, what, max_tokens=32, fixed=0, stop_reason=None):
    want, stop, wav = _single(o, ids, name, seed, max_tokens, fixed)
    s, l = lookup_ids(o.cfg, "aiden", "english")
    ctx = dict(oracle=o, ids=ids, spk=s, lang=l,
               params=dict(max_tokens=max_tokens, fixed=fixed, seed=seed, **_params(name)))
    codes_equal(got, want, f"{what} ({name}, seed {seed})", ctx)
    if stop_reason is None:   # a batch slot: it stopped at EOS iff it ended below the frame limit
        stop_reason = 1 if fixed == 0 and len(got) < max_tokens else 2
    assert stop_reason == stop, (what, name, seed, stop_reason, stop)
    _audio_close(audio, wav, f"{what} ({name}, seed {seed}) audio")


def _arm(m, plan):
    m.set_utterance_sampling([dict(SETS[name], seed=seed) for name, seed in plan])


PLAN12 = [(name, seed) for name in SETS for seed in (7, 8)]


def test_oracle_runs_differ_pairwise(tiny_eos):
    """the oracle side of the batch test is not vacuous: the twelve single runs
    of the one prompt differ pairwise -- except greedy, which no seed moves --
    and show both stop reasons, so a slot decoded with another slot's
    parameters or seed, or with rep 1.05 for 1.5, cannot pass"""
    _, o = tiny_eos
    runs = {p: _single(o, prompt_ids("short"), *p) for p in PLAN12}
    for i, a in enumerate(PLAN12):
        for b in PLAN12[i + 1:]:
            same = runs[a][0].shape == runs[b][0].shape and np.array_equal(runs[a][0], runs[b][0])
            assert same == (a[0] == "greedy" and b[0] == "greedy"), (a, b)
    assert {runs[p][1] for p in PLAN12} == {1, 2}
    assert all(12 <= len(runs[p][0]) <= 32 for p in PLAN12)


def _batch12(m, o, prompts, fixed=0, max_tokens=32):
    m.set_params(max_tokens=max_tokens, fixed=fixed, seed=42, **DEFAULT)
    _arm(m, PLAN12)
    rc, audio = m.generate_batch(prompts, ["aiden"] * 12, ["english"] * 12)
    assert rc == 0
    cap = fixed if fixed else max_tokens
    for b, (name, seed) in enumerate(PLAN12):
        _check_utt(o, m.last_codes_slot(b, cap), audio[b], prompts[b], name, seed, f"slot {b}", max_tokens, fixed)


def test_batch_12_slots_six_sets_two_seeds(tiny_eos):
    """one prompt in 12 slots, six parameter sets x seeds 7 / 8: every slot's
    codes, stop reason and audio equal its oracle single run"""
    m, o = tiny_eos
    _batch12(m, o, [prompt_ids("short")] * 12)


def test_batch_12_slots_three_prompts(tiny_eos):
    m, o = tiny_eos
    three = [prompt_ids("short"), prompt_ids("p128", 1300), prompt_ids("p128", 1301)]
    _batch12(m, o, [three[b % 3] for b in range(12)])


def test_batch_12_slots_fixed_length(tiny_eos):
    """fixed mode: the EOS redraw runs with the row's own temperature"""
    m, o = tiny_eos
    _batch12(m, o, [prompt_ids("short")] * 12, fixed=12, max_tokens=4096)


def test_armed_with_ctx_values_is_the_unarmed_run(tiny_eos, monkeypatch):
    """every row equal to the ctx's parameters: the codes and the audio bytes
    of the unarmed generate_batch, from the per-slot sampler (the counter moves
    by 16 launches per frame with launch-per-op frames); the run after it is
    plain again: the counter stands still, the codes are the unarmed ones"""
    monkeypatch.setenv("QTTS_HIP_NO_GRAPH", "1")
    m, o = tiny_eos
    prompts = [prompt_ids("short"), prompt_ids("p128", 1300), prompt_ids("p128", 1301)]
    m.set_params(max_tokens=4096, fixed=10, seed=7, **DEFAULT)
    n0 = qtts.Kernels.sample_slot_launches()
    rc, a0 = m.generate_batch(prompts, ["aiden"] * 3, ["english"] * 3)
    assert rc == 0 and qtts.Kernels.sample_slot_launches() == n0
    c0 = m.last_codes_batch(3, 10)
    m.set_utterance_sampling([{}] * 3)
    rc, a1 = m.generate_batch(prompts, ["aiden"] * 3, ["english"] * 3)
    assert rc == 0
    assert qtts.Kernels.sample_slot_launches() - n0 == 10 * m.cfg.num_code_groups
    c1 = m.last_codes_batch(3, 10)
    n1 = qtts.Kernels.sample_slot_launches()
    rc, a2 = m.generate_batch(prompts, ["aiden"] * 3, ["english"] * 3)   # the arming was one-shot
    assert rc == 0 and qtts.Kernels.sample_slot_launches() == n1
    c2 = m.last_codes_batch(3, 10)
    for b in range(3):
        np.testing.assert_array_equal(c1[b], c0[b], err_msg=f"armed slot {b}")
        assert a1[b].tobytes() == a0[b].tobytes(), b
        np.testing.assert_array_equal(c2[b], c0[b], err_msg=f"plain-again slot {b}")
        assert a2[b].tobytes() == a0[b].tobytes(), b


def test_armed_graph_frames_hold_the_per_slot_sampler(tiny_eos):
    """with frame graphs the per-slot samplers are captured (the counter moves
    at the capture), and an unarmed run right after captures the plain ones"""
    m, o = tiny_eos
    m.set_params(max_tokens=32, fixed=0, seed=42, **DEFAULT)
    n0 = qtts.Kernels.sample_slot_launches()
    _arm(m, [("default", 7), ("k300", 8)])
    rc, audio = m.generate_batch([prompt_ids("short")] * 2, ["aiden"] * 2, ["english"] * 2)
    assert rc == 0 and qtts.Kernels.sample_slot_launches() > n0
    for b, (name, seed) in enumerate([("default", 7), ("k300", 8)]):
        _check_utt(o, m.last_codes_slot(b, 32), audio[b], prompt_ids("short"), name, seed, f"slot {b}")
    n1 = qtts.Kernels.sample_slot_launches()
    m.set_params(max_tokens=32, fixed=0, seed=7, **DEFAULT)
    rc, audio = m.generate_batch([prompt_ids("short")] * 2, ["aiden"] * 2, ["english"] * 2)
    assert rc == 0 and qtts.Kernels.sample_slot_launches() == n1
    for b in range(2):
        _check_utt(o, m.last_codes_slot(b, 32), audio[b], prompt_ids("short"), "default", 7, f"plain slot {b}")


def test_wide_batch_20_slots(tiny_eos):
    """20 slots (the wide batch GEMV), the sets x seeds cycling: every slot
    equals its oracle single run"""
    m, o = tiny_eos
    plan = [PLAN12[b % 12] for b in range(20)]
    m.set_params(max_tokens=32, fixed=0, seed=42, **DEFAULT)
    w0 = qtts.Kernels.gemv_wide_launches()
    _arm(m, plan)
    rc, audio = m.generate_batch([prompt_ids("short")] * 20, ["aiden"] * 20, ["english"] * 20)
    assert rc == 0 and qtts.Kernels.gemv_wide_launches() > w0
    for b, (name, seed) in enumerate(plan):
        _check_utt(o, m.last_codes_slot(b, 32), audio[b], prompt_ids("short"), name, seed, f"slot {b}")


def _queue_prompts():
    return [prompt_ids("short"), prompt_ids("p128", 1300), prompt_ids("p128", 1301), prompt_ids("short")] + \
        [prompt_ids("p128", 1310 + i) for i in range(6)]   # test_gpu_queue._tiny_prompts()


# utterances 0 .. 4 are fast-path eligible: the frame graphs are captured with
# the fast-only family, and `nucleus` (utterance 5) is the run's first row that
# needs the full path -- it arrives by refill
QUEUE_PLAN = [("default", 7), ("greedy", 7), ("rep15", 7), ("k300", 7), ("default", 8),
              ("nucleus", 7), ("hot", 7), ("greedy", 8), ("rep15", 8), ("k300", 8)]


def _queue_check(m, o, prompts, audio):
    st = m.queue_stats()
    for i, (name, seed) in enumerate(QUEUE_PLAN):
        _check_utt(o, m.queue_codes(i), audio[i], prompts[i], name, seed, f"utterance {i} (slot {st['slot'][i]})",
                   stop_reason=st["stop_reason"][i])


def test_queue_rows_follow_their_utterances(tiny_eos):
    """10 utterances on 3 slots, each with its own set and seed: 7 refills
    start their slot from the admitted utterance's row, the first full-path
    row arrives by refill into fast-only graphs (the frames switch to the
    general kernel), and the compacted tail carries rows with move_slot"""
    m, o = tiny_eos
    assert all(name in FAST_SETS for name, _ in QUEUE_PLAN[:5]) and QUEUE_PLAN[5][0] == "nucleus"
    prompts = _queue_prompts()
    m.set_params(max_tokens=32, fixed=0, seed=42, **DEFAULT)
    _arm(m, QUEUE_PLAN)
    rc, audio = m.generate_queue(prompts, ["aiden"] * 10, ["english"] * 10, slots=3)
    assert rc == 0
    st = m.queue_stats()
    assert st["slots"] == 3 and st["refills"] == 7, st
    assert st["rows_launched"] < 3 * st["frames"], st   # the tail ran compacted
    _queue_check(m, o, prompts, audio)


def test_queue_caller_chosen_admission_order(tiny_eos):
    """per[i] belongs to utterance i in input order, whatever the admission
    order and the slot"""
    m, o = tiny_eos
    prompts = _queue_prompts()
    m.set_params(max_tokens=32, fixed=0, seed=42, **DEFAULT)
    _arm(m, QUEUE_PLAN)
    order = iter([9, 2, 7, 0, 5, 1, 8, 3, 6, 4])
    rc, audio = m.generate_queue(prompts, ["aiden"] * 10, ["english"] * 10, slots=4,
                                 next_fn=lambda: next(order, -1))
    assert rc == 0
    assert m.queue_stats()["slot"][9] == 0 and m.queue_stats()["refills"] == 6
    _queue_check(m, o, prompts, audio)


def test_refusals_leave_the_context_usable(tiny_eos):
    m, o = tiny_eos
    ids = prompt_ids("short")
    m.set_params(max_tokens=32, fixed=0, seed=7, **DEFAULT)

    def plain_ok():
        rc, audio = m.generate_batch([ids] * 2, ["aiden"] * 2, ["english"] * 2)
        assert rc == 0
        for b in range(2):
            _check_utt(o, m.last_codes_slot(b, 32), audio[b], ids, "default", 7, f"plain slot {b}")

    # n != nb (batch), n != nq (queue), n != 1 (single): -1, the arming is gone
    _arm(m, PLAN12[:3])
    rc, audio = m.generate_batch([ids] * 2, ["aiden"] * 2, ["english"] * 2)
    assert rc == -1 and all(a is None for a in audio) and not m.c.sampling
    plain_ok()
    _arm(m, PLAN12[:3])
    rc, audio = m.generate_queue([ids] * 4, ["aiden"] * 4, ["english"] * 4, slots=3)
    assert rc == -1 and all(a is None for a in audio) and not m.c.sampling
    _arm(m, PLAN12[:2])
    assert m.generate(ids, "aiden", "english") is None and not m.c.sampling
    plain_ok()
    # with forced codes as well: -1, both disarmed
    _arm(m, PLAN12[:2])
    m.force_codes(np.zeros((1, 16), np.int32), slot=0)
    rc, audio = m.generate_batch([ids] * 2, ["aiden"] * 2, ["english"] * 2)
    assert rc == -1 and not m.c.sampling and not m.c.force
    plain_ok()
    # the device level: a bad slot, bad values, and forcing after the table is armed
    dev = C.c_void_p(m.c.hip)
    lib = qtts.lib()
    good = qtts.SlotParams(0.9, 1.0, 1.05, 50, 0.9, 1.0, 50, 42)
    for b in (-1, 2, 64):
        assert lib.qtts_dev_slot_params(dev, b, C.byref(good)) == -1
    for field, v in (("top_p", 0.0), ("repetition_penalty", 0.0), ("temperature", float("nan")),
                     ("st_top_p", float("inf"))):
        bad = qtts.SlotParams(0.9, 1.0, 1.05, 50, 0.9, 1.0, 50, 42)
        setattr(bad, field, v)
        assert lib.qtts_dev_slot_params(dev, 0, C.byref(bad)) == -1
    plain_ok()
    # per-slot parameters and forcing on one run: whichever is armed second is refused

    class GenParams(C.Structure):   # qtts_gen_params_t
        _fields_ = [("temperature", C.c_float), ("top_p", C.c_float), ("repetition_penalty", C.c_float),
                    ("top_k", C.c_int), ("st_temperature", C.c_float), ("st_top_p", C.c_float), ("st_top_k", C.c_int),
                    ("fixed_codec_tokens", C.c_int), ("seed", C.c_int)]
    gp = GenParams(0.9, 1.0, 1.05, 50, 0.9, 1.0, 50, 0, 7)
    codes = (C.c_int * 16)(*([0] * 16))
    assert lib.qtts_dev_begin(dev, 2, 32, 16, C.byref(gp)) == 0
    assert lib.qtts_dev_slot_params(dev, 1, C.byref(good)) == 0
    assert lib.qtts_dev_force(dev, 0, codes, 1) == -1 and lib.qtts_dev_tap(dev, 0, 0, 0) == -1
    assert lib.qtts_dev_begin(dev, 2, 32, 16, C.byref(gp)) == 0          # (disarms the table)
    assert lib.qtts_dev_force(dev, 0, codes, 1) == 0
    assert lib.qtts_dev_slot_params(dev, 1, C.byref(good)) == -1
    plain_ok()                                                           # the next begin disarms either


# ---------------------------------------------------------------- 7. the synthetic 1.7B
@pytest.mark.slow
def test_17b_four_slots_equal_their_single_runs(gpu):
    """4 slots x 8 frames on the synthetic 1.7B, four sets and seeds: each
    slot's codes equal the same utterance's single run on the ctx-wide path
    with that set (a differing draw gets tests/parity.py's verdict)"""
    md = model_dir("1.7b")
    m = qtts.QwenTTS(md)
    try:
        plan = [("default", 42), ("nucleus", 7), ("k300", 8), ("hot", 9)]
        prompts = [prompt_ids("short"), prompt_ids("p128", 1300), prompt_ids("p128", 1301), prompt_ids("short")]
        single = []
        for (name, seed), ids in zip(plan, prompts):
            m.set_params(max_tokens=4096, fixed=8, seed=seed, **_params(name))
            assert m.generate(ids, "aiden", "english") is not None
            single.append(m.last_codes())
        m.set_params(max_tokens=4096, fixed=8, seed=42, **DEFAULT)
        _arm(m, plan)
        rc, _ = m.generate_batch(prompts, ["aiden"] * 4, ["english"] * 4)
        assert rc == 0
        got = m.last_codes_batch(4, 8)
        if any(not np.array_equal(got[b], single[b]) for b in range(4)):   # (the verdict needs the oracle)
            o = Oracle(md)
            s, l = lookup_ids(o.cfg, "aiden", "english")
            for b, (name, seed) in enumerate(plan):
                ctx = dict(oracle=o, ids=prompts[b], spk=s, lang=l,
                           params=dict(max_tokens=4096, fixed=8, seed=seed, **_params(name)))
                codes_equal(got[b], single[b], f"1.7B slot {b} ({name}, seed {seed})", ctx)
    finally:
        m.close()


# ---------------------------------------------------------------- 8. the CLI
def test_cli_seed_step_writes_every_take(tiny_eos):
    """--batch 3 --seed-step 1 writes three WAVs; slot b's is byte-equal to a
    --batch 1 --seed <seed + b> run's"""
    md = model_dir("tiny", eos_gain=manifest()["eos_gain"])
    ids = ",".join(str(i) for i in prompt_ids("short"))
    base = [qtts.CLI_PATH, "-d", md, "-t", ids, "-s", "aiden", "-l", "english", "--max-tokens", "32"]
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(base + ["-o", os.path.join(d, "take.wav"), "--seed", "7", "--batch", "3", "--seed-step", "1"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        takes = [open(os.path.join(d, n), "rb").read() for n in ("take.wav", "take_1.wav", "take_2.wav")]
        assert len(set(takes)) == 3
        for b in range(3):
            r = subprocess.run(base + ["-o", os.path.join(d, f"one{b}.wav"), "--seed", str(7 + b)],
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            assert open(os.path.join(d, f"one{b}.wav"), "rb").read() == takes[b], b
        assert sorted(os.listdir(d)) == ["one0.wav", "one1.wav", "one2.wav", "take.wav", "take_1.wav", "take_2.wav"]
