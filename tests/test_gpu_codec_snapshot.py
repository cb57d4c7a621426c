"""Save and restore of one multi-stream codec stream's carried state
(qwen_tts_codec_mstream_save / _restore): the 21 history planes, K/V rows
0..hl-1 of every layer, the position and hl, in a compact snapshot that any
stream of any later begin takes over in one launch.

Three streams are primed by one ragged push with references of 7, 63 and 90
frames: hl well below the tiny codec's window of 72, one pass of 16 below it,
and the full 71 rows after the window has run over.

Bounds are the multi-stream codec's: bit identity wherever two runs do the
same arithmetic, 1e-5 max-abs against the full decode of the same codes on the
device, audio_close (1e-4) against the oracle.
"""
import numpy as np
import pytest

import qtts
from test_gpu_codec_mstream_ragged import audio_close, full_decode

pytestmark = pytest.mark.gpu

REFS = [7, 63, 90]
T, CAP = 3, 128
_rng = np.random.default_rng(77)
REF = [_rng.integers(0, 2048, size=(n, 16)).astype(np.int32) for n in REFS]
X = _rng.integers(0, 2048, size=(3, T, 16)).astype(np.int32)          # what every voice continues with
JUNK = _rng.integers(0, 2048, size=(3, 20, 16)).astype(np.int32)


def prime(m, n_streams=3, cap=CAP):
    """begin, then the three references in one ragged push: streams 0..2 at 7 / 63 / 90 frames"""
    assert m.codec_mstream_begin(n_streams, cap) == 0
    assert m.codec_mstream_push_ragged([0, 1, 2], REF) is not None
    assert [m.codec_mstream_pos(s) for s in range(3)] == REFS


_BASE = {}


def baseline(m):
    """the three voices continued by X in one push, and voice 0 continued alone, no save anywhere"""
    if not _BASE:
        prime(m)
        _BASE["all"] = m.codec_mstream_push_any([0, 1, 2], X)
        prime(m)
        _BASE["alone0"] = m.codec_mstream_push_any([0], X[:1])[0]
    return _BASE


def save_all(m):
    snaps = [m.codec_mstream_save(s) for s in range(3)]
    assert all(snaps)
    assert [m.codec_snapshot_pos(p) for p in snaps] == REFS
    return snaps


def free_all(m, snaps):
    for p in snaps:
        m.codec_snapshot_free(p)


def test_restore_equals_continuing_and_save_does_not_disturb(tts_tiny, oracle):
    m = tts_tiny
    base = baseline(m)
    prime(m)
    snaps = save_all(m)
    a = m.codec_mstream_push_any([0, 1, 2], X)
    for v in range(3):      # the source streams went on as if nothing had been saved
        np.testing.assert_array_equal(a[v], base["all"][v])
    for s in range(3):
        assert m.codec_mstream_reset(s) == 0
    assert m.codec_mstream_push_any([0, 1, 2], JUNK) is not None
    where = [2, 0, 1]       # voice v's snapshot goes to stream where[v]
    for v in range(3):
        assert m.codec_mstream_restore(where[v], snaps[v]) == 0
        assert m.codec_mstream_pos(where[v]) == REFS[v]
    b = m.codec_mstream_push_any(where, X)      # voice v is again the v-th stream of the push
    assert [m.codec_mstream_pos(where[v]) for v in range(3)] == [n + T for n in REFS]
    for v in range(3):
        np.testing.assert_array_equal(a[v], b[v])
        full = oracle.codec_decode(np.concatenate([REF[v], X[v]]))
        audio_close(b[v], full[REFS[v] * 1920:])
    free_all(m, snaps)


def test_a_restored_stream_does_not_see_stale_rows(tts_tiny):
    m = tts_tiny
    base = baseline(m)
    prime(m)
    snaps = save_all(m)
    # stream 2 sits at 90 frames: all 71 K/V rows written; the 7-frame voice brings 7 of them
    assert m.codec_mstream_restore(2, snaps[0]) == 0
    assert m.codec_mstream_pos(2) == 7
    got = m.codec_mstream_push_any([2], X[:1])[0]
    np.testing.assert_array_equal(got, base["alone0"])
    free_all(m, snaps)


def test_a_snapshot_survives_a_begin_with_another_stream_count(tts_tiny):
    m = tts_tiny
    prime(m)
    snaps = save_all(m)
    assert m.codec_mstream_begin(5, 200) == 0
    assert m.codec_mstream_restore(4, snaps[1]) == 0 and m.codec_mstream_restore(1, snaps[2]) == 0
    assert m.codec_mstream_pos(4) == 63 and m.codec_mstream_pos(1) == 90 and m.codec_mstream_pos(0) == 0
    out = m.codec_mstream_push_any([4, 1], X[1:3])
    worst = 0.0
    for got, v in zip(out, (1, 2)):
        full = full_decode(m, np.concatenate([REF[v], X[v]]))[REFS[v] * 1920:]
        assert got.shape == full.shape
        worst = max(worst, float(np.abs(got - full).max()))
    print(f"measured  restored under 5 streams: largest |stream - full decode| {worst:.3e}")
    assert worst < 1e-5, worst
    free_all(m, snaps)


def test_refusals_leave_the_state_untouched(tts_tiny, tiny_dir, capfd):
    m = tts_tiny
    base = baseline(m)
    other = qtts.QwenTTS(tiny_dir)
    try:
        capfd.readouterr()
        # no begin on a context that never began
        assert other.codec_mstream_save(0) is None
        assert "save without begin" in capfd.readouterr().err
        prime(other)
        foreign = other.codec_mstream_save(0)
        assert foreign

        prime(m)
        snaps = save_all(m)
        freed = m.codec_mstream_save(1)
        m.codec_snapshot_free(freed)
        assert m.codec_snapshot_pos(freed) == -1
        capfd.readouterr()
        for s in (-1, 3):                                   # a bad stream
            assert m.codec_mstream_save(s) is None
            assert "out of range" in capfd.readouterr().err
            assert m.codec_mstream_restore(s, snaps[0]) == -1
            assert "out of range" in capfd.readouterr().err
        assert m.codec_mstream_restore(0, None) == -1       # NULL
        assert "got NULL" in capfd.readouterr().err
        assert m.codec_mstream_restore(0, freed) == -1      # freed
        assert "a freed one" in capfd.readouterr().err
        assert m.codec_mstream_restore(0, foreign) == -1    # saved on a second context
        assert "another context" in capfd.readouterr().err
        assert [m.codec_mstream_pos(s) for s in range(3)] == REFS
        assert [m.codec_snapshot_pos(p) for p in snaps] == REFS
        a = m.codec_mstream_push_any([0, 1, 2], X)
        for v in range(3):
            np.testing.assert_array_equal(a[v], base["all"][v])

        # a position beyond max_frames: 90 frames into streams that hold 64
        def short(refuse):
            assert m.codec_mstream_begin(3, 64) == 0
            assert m.codec_mstream_push_any([0, 1], JUNK[:2, :5]) is not None
            if refuse:
                capfd.readouterr()
                assert m.codec_mstream_restore(0, snaps[2]) == -1
                assert "exceed the stream capacity 64" in capfd.readouterr().err
                assert m.codec_mstream_pos(0) == 5
                assert m.codec_mstream_restore(1, snaps[1]) == 0     # (63 frames fit)
            return m.codec_mstream_push_any([0], X[:1])[0]
        np.testing.assert_array_equal(short(True), short(False))

        # a context's snapshots die with it: refused afterwards, and still freeable
        other.close()
        assert m.codec_snapshot_pos(foreign) == -1
        assert m.codec_mstream_restore(0, foreign) == -1
        assert "a context that was freed" in capfd.readouterr().err
        m.codec_snapshot_free(foreign)
        m.codec_snapshot_free(foreign)      # (a freed pointer: nothing happens)
        free_all(m, snaps)
    finally:
        other.close()
