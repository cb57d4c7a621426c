#!/usr/bin/env python3
"""Codec snapshots, voice handles and the voice-clone work queue on the
synthetic 1.7B model (measurement tool).

  python3 tools/prof_voice_queue.py [--reps 3] [--parent-lib PATH] [--out profiles/voice_queue_bench.txt]

Every figure is the median over --reps fresh processes (one child process per
repetition and quantity; the sides of a comparison alternate inside each
repetition).

  restore  n streams (1, 8) taken to a primed state of 63 reference frames,
           host wall including a device sync (ms, the median over 10 rounds):
             restore  n x qwen_tts_codec_mstream_restore of saved snapshots
                      (each round after a reset of the streams)
             prime    the same references pushed through the codec from
                      position 0 -- push_any at n = 1, one push_ragged at n = 8 --
                      on the build --parent-lib names (the parent commit's)
                      where given, else on this build
           and one snapshot's device bytes
  queue    96 EOS utterances (bench.py --eos --queue 96's prompts) over 8
           voices of 63 reference frames on 8 slots, chunk_frames 4, through
           qwen_tts_generate_voice_queue_stream, called twice on the same
           handles (the first call primes and saves the 8 voices, the second
           only restores): audio-s/s, slot occupancy, every utterance's first
           packet from its admission (`next`) to its first chunk (median and
           p95, the refilled utterances separately); beside it
           qwen_tts_generate_voice_queue (plain) and, in lock step on the first
           8 utterances, qwen_tts_generate_voice_clone_batch_stream
  bench    bench.py --gpus 1 --steps 3 --warmup 1 [--batch 8] on this build and
           on the parent's (the unchanged paths)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "qwen3-tts-c_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
EOS_GAIN = 1.4      # bench.py --eos
NREF = 63


def _model(eos=False):
    import qtts
    from synth_model import ensure_model
    base = os.environ.get("QTTS_TEST_MODELS", "/tmp/qtts_test_models")
    if eos:         # the directory bench.py --eos uses
        md = ensure_model(os.path.join(base, f"1.7b_eos_gain{EOS_GAIN}"), "1.7b", overrides={"eos_gain": EOS_GAIN})
    else:
        md = ensure_model(os.path.join(base, "1.7b"), "1.7b")
    return qtts.QwenTTS(md)


def child_restore(side, n):
    """{ms}: n streams to the state after 63 reference frames, host wall with a device sync"""
    import numpy as np
    import qtts
    m = _model()
    sync = qtts.lib().qtts_hip_sync
    rng = np.random.default_rng(n)
    codes = [rng.integers(0, 2048, size=(NREF, 16)).astype(np.int32) for _ in range(n)]
    warm, reps = 3, 10
    ts, res = [], {}
    assert m.codec_mstream_begin(n, 256) == 0
    if side == "restore":
        assert m.codec_mstream_push_ragged(np.arange(n), codes) is not None
        snaps = [m.codec_mstream_save(s) for s in range(n)]
        assert all(snaps)
        res["snapshot_bytes"] = int(qtts.lib().qtts_dev_codec_snapshot_bytes(snaps[0]))
    for _ in range(warm + reps):
        for s in range(n):
            assert m.codec_mstream_reset(s) == 0
        sync()
        t0 = time.perf_counter()
        if side == "restore":
            for s in range(n):
                assert m.codec_mstream_restore(s, snaps[s]) == 0
        elif n == 1:
            assert m.codec_mstream_push_any([0], codes[0][None]) is not None
        else:
            assert m.codec_mstream_push_ragged(np.arange(n), codes) is not None
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    m.close()
    res["ms"] = statistics.median(ts[warm:])
    return res


def _voices(m, nv):
    import numpy as np
    out = []
    for i in range(nv):        # bench.py --voice-clone --vc-codes' inputs
        r = np.random.default_rng(1234 + i + 7)
        codes = r.integers(0, 2048, size=(NREF, m.cfg.num_code_groups)).astype(np.int32)
        rids = [151644, 77091, 198] + r.integers(1000, 100000, size=20).tolist() + [151645, 198]
        out.append((rids, codes, (r.standard_normal(m.cfg.talker_hidden) * 0.05).astype(np.float32)))
    return out


def child_queue(mode, nq=96, slots=8, chunk=4, nv=8):
    from oracle_py import DEFAULT
    from synth_model import prompt_ids
    m = _model(eos=True)
    m.set_params(max_tokens=4096, fixed=0, seed=42, **DEFAULT)
    n = slots if mode == "batch_stream" else nq
    ids = [prompt_ids("p128", seed=1234 + i) for i in range(n)]
    lang = ["english"] * n
    vin = _voices(m, nv)
    res = {}

    def finish(res, audio, wall, queue):
        secs = sum(len(a) for a in audio) / 24000.0
        res.update(audio_s_per_s=secs / wall, total_ms=wall * 1e3, codec_ms=float(m.c.perf_codec_ms), audio_s=secs)
        if queue:
            st = m.queue_stats()
            res.update(occupancy=st["occupancy"], frames=st["frames"], refills=st["refills"])
        else:
            fr = [len(a) // 1920 for a in audio]
            res.update(occupancy=sum(fr) / (len(fr) * (max(fr) + 1)), frames=max(fr))
        return res

    if mode == "batch_stream":
        v = [vin[i % nv] for i in range(n)]
        for _ in range(2):      # the second request is the one reported
            t0 = time.perf_counter()
            rc, audio = m.generate_voice_clone_batch_stream(ids, [x[0] for x in v], [x[1] for x in v],
                                                            [x[2] for x in v], lang, chunk_frames=chunk)
            wall = time.perf_counter() - t0
            assert rc == 0 and all(a is not None for a in audio)
        res.update(first_packet_ms=float(m.c.perf_first_packet_ms))
        finish(res, audio, wall, False)
    else:
        hs = [m.voice_create(*v) for v in vin]
        assert all(hs)
        voices = [hs[i % nv] for i in range(n)]
        for call in ("first", "second"):
            seq, admitted, first = iter(range(n)), {}, {}

            def next_fn():
                u = next(seq, -1)
                admitted[u] = time.perf_counter()
                return u

            def on_chunk(u, a):
                if u not in first:
                    first[u] = time.perf_counter()
            t0 = time.perf_counter()
            if mode == "queue":
                rc, audio = m.generate_voice_queue(ids, voices, lang, slots=slots, next_fn=next_fn)
            else:
                rc, audio = m.generate_voice_queue_stream(ids, voices, lang, slots=slots, next_fn=next_fn,
                                                          chunk_frames=chunk, on_chunk=on_chunk)
            wall = time.perf_counter() - t0
            assert rc == 0 and all(a is not None for a in audio)
            r = {"primed_after": sum(m.voice_info(h)["primed"] for h in hs)}
            if mode == "queue_stream":
                # (the first `slots` admissions wait for the prompts' prefill; the refills are the steady state)
                lat = sorted((first[u] - admitted[u]) * 1e3 for u in first)
                refl = sorted((first[u] - admitted[u]) * 1e3 for u in first if u >= slots)
                r.update(fp_median_ms=statistics.median(lat), fp_p95_ms=lat[min(len(lat) - 1, int(0.95 * len(lat)))],
                         fp_refill_median_ms=statistics.median(refl),
                         fp_refill_p95_ms=refl[min(len(refl) - 1, int(0.95 * len(refl)))],
                         first_packet_ms=float(m.c.perf_first_packet_ms))
            res[call] = finish(r, audio, wall, True)
        for h in hs:
            m.voice_free(h)
    m.close()
    return res


def spawn(args, lib=None):
    env = dict(os.environ)
    if lib:
        env["QTTS_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=900, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"child {args} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def bench(extra, lib=None):
    env = dict(os.environ)
    if lib:
        env["QTTS_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"]
                       + extra, capture_output=True, text=True, timeout=900, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py {extra} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    for line in reversed(r.stdout.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise RuntimeError("bench.py printed no result line")


def med(rows, key):
    v = [r[key] for r in rows if r.get(key) is not None]
    return statistics.median(v) if v else float("nan")


def each(rows, key, fmt="{:.3f}"):
    return " ".join(fmt.format(r[key]) for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs="+")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libqwen_tts_amd.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voice_queue_bench.txt"))
    ap.add_argument("--only", default="restore,queue,bench", help="comma list of restore, queue, bench")
    ap.add_argument("--append", action="store_true", help="append to --out instead of rewriting it")
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "restore":
            print(json.dumps(child_restore(a.child[1], int(a.child[2]))))
        else:
            print(json.dumps(child_queue(a.child[1])))
        return
    only = a.only.split(",")
    where = "the parent commit's build" if a.parent_lib else "this build"
    with open(a.out, "a" if a.append else "w") as f:
        f.write(f"# tools/prof_voice_queue.py --reps {a.reps} --only {a.only}: medians over {a.reps} fresh processes, "
                "synthetic 1.7B\n")

    def say(s):     # (written as it goes: a run cut short keeps what it measured)
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    if "restore" in only:
        for n in (1, 8):
            rows = {"restore": [], "prime": []}
            for _ in range(a.reps):
                rows["restore"].append(spawn(["restore", "restore", n]))
                rows["prime"].append(spawn(["restore", "prime", n], a.parent_lib))
            rs, pr = med(rows["restore"], "ms"), med(rows["prime"], "ms")
            how = "push_any" if n == 1 else "one push_ragged"
            say(f"restore n={n} x {NREF} reference frames, host wall with a sync: {n} restore {rs:7.3f} ms "
                f"({each(rows['restore'], 'ms')})   priming by {how} on {where} {pr:7.3f} ms "
                f"({each(rows['prime'], 'ms')})   ratio {pr / rs:.1f}x   snapshot "
                f"{rows['restore'][0]['snapshot_bytes'] / 1e6:.2f} MB")
    if "queue" in only:
        plan = ["queue_stream", "queue", "batch_stream"]
        rows = {p: [] for p in plan}
        for _ in range(a.reps):
            for p in plan:
                rows[p].append(spawn(["queue", p]))
        for p in ("queue_stream", "queue"):
            for call in ("first", "second"):
                r = [x[call] for x in rows[p]]
                fp = ""
                if p == "queue_stream":
                    fp = (f"   first packet per utterance: median {med(r, 'fp_median_ms'):6.2f} ms p95 "
                          f"{med(r, 'fp_p95_ms'):6.2f} ms, refilled only: median {med(r, 'fp_refill_median_ms'):6.2f} ms "
                          f"({each(r, 'fp_refill_median_ms', '{:.2f}')}) p95 {med(r, 'fp_refill_p95_ms'):6.2f} ms; "
                          f"the call's first packet {med(r, 'first_packet_ms'):7.2f} ms "
                          f"({each(r, 'first_packet_ms', '{:.2f}')})")
                say(f"voice {p:12s} {call:6s} call, 96 EOS utterances over 8 voices x {NREF} frames on 8 slots, chunk 4: "
                    f"{med(r, 'audio_s_per_s'):7.1f} audio-s/s ({each(r, 'audio_s_per_s', '{:.1f}')})   occupancy "
                    f"{med(r, 'occupancy'):.3f}   {int(med(r, 'frames'))} frames, {int(med(r, 'refills'))} refills, "
                    f"{med(r, 'audio_s'):.1f} s audio in {med(r, 'total_ms'):7.1f} ms (codec {med(r, 'codec_ms'):6.1f} ms)   "
                    f"handles primed afterwards {int(med(r, 'primed_after'))}{fp}")
        r = rows["batch_stream"]
        say(f"voice batch_stream lock step on the first 8 utterances, chunk 4: {med(r, 'audio_s_per_s'):7.1f} audio-s/s "
            f"({each(r, 'audio_s_per_s', '{:.1f}')})   occupancy {med(r, 'occupancy'):.3f}   {int(med(r, 'frames'))} "
            f"frames, {med(r, 'audio_s'):.1f} s audio in {med(r, 'total_ms'):7.1f} ms   first packet "
            f"{med(r, 'first_packet_ms'):7.2f} ms ({each(r, 'first_packet_ms', '{:.2f}')})")
    if "bench" in only:
        for extra in ([], ["--batch", "8"]):
            rows = {"parent": [], "this": []}
            for _ in range(a.reps):
                rows["parent"].append(bench(extra, a.parent_lib))
                rows["this"].append(bench(extra))
            key = "value" if "value" in rows["this"][0] else "audio_s_per_s"
            p, t = med(rows["parent"], key), med(rows["this"], key)
            say(f"bench.py --gpus 1 --steps 3 --warmup 1 {' '.join(extra):9s}: {where} {p:7.2f} ({each(rows['parent'], key, '{:.2f}')})"
                f"   this build {t:7.2f} ({each(rows['this'], key, '{:.2f}')}) audio-s/s   {100 * (t / p - 1):+.1f} %")


if __name__ == "__main__":
    main()
