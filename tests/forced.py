"""Two-sided verdict on a draw that differs from the reference under the
reference's own history (TEST INFRASTRUCTURE).

A run with the reference's codes forced (qwen_tts_force_codes) keeps, per
draw, the id the sampler itself produced (qwen_tts_last_drawn).  Where that id
is not the reference's, tests/divergence.py asks how close the REFERENCE's
draw was to flipping (eps_flip against the head GEMV's rounding bound
eps_gemv).  That side alone would also excuse a wrong kernel that happens to
land on a near-tie, so this module adds the GPU's side from a logit tap of the
same draw (qwen_tts_tap_draw): over the candidate ids -- the only logits the
draw's outcome depends on --

    max |tap_logits - oracle_logits| <= CARRY * eps_gemv

i.e. the GPU's logits differ from the reference's by no more than the rounding
the reference-side verdict appeals to (the head's own bound, times the same
allowance for the rounding its input row carries).  The verdict is a near-tie
only if both sides hold.
"""
import numpy as np

from divergence import CARRY, classify, gemv_bound, flip_distance


def sampling_of(params, group):
    """(top_k, top_p, temperature) of draw group `group` under the oracle's keyword parameters"""
    if group == 0:
        return params.get("top_k", 50), params.get("top_p", 1.0), params.get("temperature", 0.9)
    return params.get("st_top_k", 50), params.get("st_top_p", 1.0), params.get("st_temperature", 0.9)


def classify_two_sided(oracle, tap, ids, spk, lang, frame, group, params):
    """tap: (logits, rng_bits, drawn) of the GPU's draw (frame, group) under the
    reference's history (QwenTTS.tap_result).  Returns the reference-side
    fields of divergence.classify (verdict_ref, eps_flip, eps_gemv, ratio_ref)
    plus the GPU side: gpu_err = max |tap - oracle| over the candidate ids and
    the drawn id, ratio_gpu = gpu_err / (CARRY * eps_gemv), and
    verdict = "fp near-tie" iff the reference side says near-tie (carried or
    not) and ratio_gpu <= 1, else "bug"."""
    lg_gpu, _, drawn = tap
    ref = classify(oracle, ids, spk, lang, frame, group, params, got=int(drawn))
    if ref.get("verdict") == "unclassified":
        return dict(verdict="unclassified", why=ref.get("why"))
    tr = oracle.trace_draw(ids, spk, lang, frame, group, **params)
    tk, tp, tt = sampling_of(params, group)
    cand = flip_distance(tr["logits"], tk, tp, tt, tr["rng_bits"])["candidates"]
    rows = sorted(set(cand) | {int(drawn)})
    lg_gpu = np.asarray(lg_gpu, np.float64)
    lg_ref = np.asarray(tr["logits"], np.float64)
    assert lg_gpu.shape == lg_ref.shape, (lg_gpu.shape, lg_ref.shape)
    gpu_err = float(np.abs(lg_gpu[rows] - lg_ref[rows]).max())
    eps_gemv = float(gemv_bound(oracle.tensors, group, tr["x"], rows).max())
    assert eps_gemv == ref["eps_gemv"], (eps_gemv, ref["eps_gemv"])   # the same rows, the same bound
    ratio_gpu = gpu_err / (CARRY * eps_gemv)
    both = ref["verdict"].startswith("fp near-tie") and ratio_gpu <= 1.0
    return dict(verdict="fp near-tie" if both else "bug", verdict_ref=ref["verdict"], frame=int(frame),
                group=int(group), reference=int(ref["reference"]), drawn=int(drawn),
                eps_flip=float(ref["eps_flip"]), eps_gemv=eps_gemv, ratio_ref=float(ref["ratio"]),
                gpu_err=gpu_err, ratio_gpu=float(ratio_gpu))
