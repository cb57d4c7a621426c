"""Instruct and the instruct prefix cache at the drop-in boundary, on a CPU box:
the library exports and the headers declare the new entry points, the ctypes
signatures load, the ctx mirror has the library's layout, the arming refuses a
missing handle and bad lists, qwen_tts_instruct_prompt equals transformers'
Qwen2Tokenizer on the instruct's chat template, and the CLI lists both flags."""
import ctypes as C
import json
import os
import re
import subprocess
import unicodedata

import pytest

import qtts

HOST = ["qwen_tts_set_utterance_instruct", "qwen_tts_instruct_prompt"]
DEV = ["qtts_dev_prefix_cache", "qtts_dev_prefix_cache_bytes", "qtts_hip_prefix_hits", "qtts_hip_prefix_misses",
       "qtts_hip_prefill_rows", "qtts_dev_get_hidden"]
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
IM_START, IM_END = 151644, 151645


def _list(*entries):
    return (C.c_char_p * len(entries))(*entries)


def test_library_exports_and_headers_declare_the_symbols():
    lib = qtts.lib()
    missing = [s for s in HOST + DEV if not hasattr(lib, s)]
    assert not missing, missing
    assert set(HOST + DEV) <= set(qtts.EXPORTS)
    for header, names in (("qwen_tts.h", HOST), ("qtts_hip.h", DEV)):
        txt = open(os.path.join(INCLUDE, header)).read()
        for s in names:
            assert re.search(r"^(int|long long|size_t|char \*) ?%s\(" % s, txt, re.M), (header, s)


def test_ctypes_signatures_load_and_ctx_mirror_matches():
    lib = qtts.lib()
    ctx = C.POINTER(qtts.Ctx)
    want = {"qwen_tts_set_utterance_instruct": (C.c_int, [ctx, C.c_int, C.POINTER(C.c_char_p)]),
            "qwen_tts_instruct_prompt": (C.c_void_p, [ctx, C.c_char_p]),
            "qtts_dev_prefix_cache": (C.c_int, [C.c_void_p, C.c_int]),
            "qtts_dev_prefix_cache_bytes": (C.c_size_t, [C.c_void_p]),
            "qtts_dev_get_hidden": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
            "qtts_hip_prefix_hits": (C.c_longlong, []),
            "qtts_hip_prefix_misses": (C.c_longlong, []),
            "qtts_hip_prefill_rows": (C.c_longlong, [])}
    for name, (res, args) in want.items():
        f = getattr(lib, name)
        assert f.restype is res and list(f.argtypes or []) == args, name
    # the arming lives behind one pointer in front of `sampling`; `force` stays the last field
    names = [n for n, _ in qtts.Ctx._fields_]
    assert names[-3:] == ["instruct", "sampling", "force"]
    assert lib.qwen_tts_abi_sizeof_ctx() == C.sizeof(qtts.Ctx)
    assert qtts.Ctx.force.offset + C.sizeof(C.c_void_p) == C.sizeof(qtts.Ctx)
    for f in ("set_utterance_instruct", "instruct_prompt", "prefix_cache", "prefix_cache_bytes", "prefix_counters"):
        assert callable(getattr(qtts.QwenTTS, f)), f
    # (callable without a device)
    assert lib.qtts_hip_prefix_hits() >= 0 and lib.qtts_hip_prefix_misses() >= 0 and lib.qtts_hip_prefill_rows() >= 0
    assert lib.qtts_dev_prefix_cache(None, 4) == -1 and lib.qtts_dev_prefix_cache_bytes(None) == 0


def test_arming_refuses_a_missing_handle():
    lib = qtts.lib()
    one = _list(b"1,2,3")
    assert lib.qwen_tts_set_utterance_instruct(None, 1, one) == -1
    ctx = qtts.Ctx()   # a ctx without a device model
    assert lib.qwen_tts_set_utterance_instruct(C.byref(ctx), 1, one) == -1
    assert not ctx.instruct and not ctx.sampling and not ctx.force
    assert not lib.qwen_tts_instruct_prompt(None, b"calm")
    assert not lib.qwen_tts_instruct_prompt(C.byref(ctx), None)


def test_arming_validation():
    """validated at arming time, before any device is needed: a ctx whose device
    handle is a dummy is never dereferenced by the arming entry"""
    lib = qtts.lib()
    ctx = qtts.Ctx()
    ctx.hip = 1   # (only tested for NULL here; no generation call follows)
    ctx.config.talker_text_vocab = 1000
    arm = lambda n, lst: lib.qwen_tts_set_utterance_instruct(C.byref(ctx), n, lst)
    for n in (0, -1):
        assert arm(n, _list(b"1,2")) == -1
    assert arm(1, None) == -1
    for bad in (b"1,x,3", b"abc", b"1,2,1000", b"-1", b"5,999999"):   # unparsable; out of [0, vocab)
        assert arm(1, _list(bad)) == -1, bad
        assert arm(3, _list(b"1,2", bad, None)) == -1, bad   # one bad entry refuses the whole list
        assert not ctx.instruct
    assert arm(2, _list(b"0,999", b" 7, 8 ,9")) == 0 and ctx.instruct
    first = ctx.instruct
    assert arm(1, _list(b"1,2,1000")) == -1 and ctx.instruct == first   # an earlier arming survives a refused one
    assert arm(3, _list(None, b"", None)) == 0 and ctx.instruct          # an all-NULL (or empty) list arms
    assert not ctx.sampling and not ctx.force
    # (the dummy ctx is Python's, never qwen_tts_free'd: its last arming, a few dozen bytes, stays allocated)


@pytest.fixture(scope="module")
def hf_tok(tiny_dir):
    from transformers import Qwen2Tokenizer
    with open(os.path.join(tiny_dir, "vocab.json"), encoding="utf-8") as f:
        v = json.load(f)
    with open(os.path.join(tiny_dir, "merges.txt"), encoding="utf-8") as f:
        m = [tuple(l.rstrip("\n").split(" ")) for l in f if not l.startswith("#version")]
    return Qwen2Tokenizer(vocab=v, merges=m)


def test_instruct_prompt_equals_transformers(tiny_dir, hf_tok):
    """"<|im_start|>user\\n{instruct}<|im_end|>\\n": the added tokens split first,
    the pieces between them go through the BPE"""
    lib = qtts.lib()
    ctx = qtts.Ctx()   # the tokenizer needs the model dir alone
    ctx.model_dir = tiny_dir.encode()
    plain = lambda s: hf_tok(s, add_special_tokens=False)["input_ids"]
    for text in ("Speak slowly, in a calm and warm voice.", "A young woman, cheerful; fast pace!", "", "  whisper\n",
                 "naïve façade 🙂 的一是"):
        text = unicodedata.normalize("NFC", text)
        p = lib.qwen_tts_instruct_prompt(C.byref(ctx), text.encode("utf-8"))
        assert p, text
        got = [int(t) for t in C.string_at(p).decode().split(",")]
        qtts._libc.free(C.c_void_p(p))
        assert got == [IM_START] + plain("user\n" + text) + [IM_END] + plain("\n"), text
        assert got == qtts.tokenize(tiny_dir, f"<|im_start|>user\n{text}<|im_end|>\n")


def test_cli_help_lists_the_instruct_flags():
    r = subprocess.run([qtts.CLI_PATH, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--instruct " in r.stdout + r.stderr and "--instruct-ids" in r.stdout + r.stderr
