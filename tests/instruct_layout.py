"""The prompt layout of an utterance with an instruct, restated for the tests
(test infrastructure): what qwen_tts.c hands to qtts_dev_prompt.  The trace
test checks it against the host's logged calls; the prefix-cache test drives
the device with it."""
TTS_PAD, TTS_BOS, TTS_EOS = 151671, 151672, 151673


def layout(cfg, ids, speaker, language, ins, b):
    """(text ids, plan rows, p_len, n_trailing) of one utterance on slot b: the
    streaming prompt layout with the instruct rows in front (DESIGN.md "Instruct and the prefix cache", Layout)"""
    tc = cfg["talker_config"]
    spk = {k.lower(): v for k, v in tc["spk_id"].items()}.get((speaker or "").lower(), -1)
    lang = -1
    if language and language.lower() != "auto":
        lang = {k.lower(): v for k, v in tc["codec_language_id"].items()}.get(language.lower(), -1)
    if lang < 0:
        prefix = [tc["codec_nothink_id"], tc["codec_think_bos_id"], tc["codec_think_eos_id"]]
    else:
        prefix = [tc["codec_think_id"], tc["codec_think_bos_id"], lang, tc["codec_think_eos_id"]]
    if spk >= 0:
        prefix.append(spk)
    prefix += [tc["codec_pad_id"], tc["codec_bos_id"]]
    np_ = len(prefix)
    nt = max(len(ids) - 4 - 5 + 1, 1)
    text = ids[:3] + [TTS_PAD, TTS_BOS, TTS_EOS, ids[3]] + ids[4:4 + nt - 1]
    n_own, ni = len(text), len(ins)
    text = text + list(ins)
    plan = [[n_own + i, -1, 2, b, i] for i in range(ni)]
    plan += [[i, -1, 0, b, ni + i] for i in range(3)]
    plan += [[3 if i < np_ - 2 else 4, prefix[i], 0, b, ni + 3 + i] for i in range(np_ - 1)]
    plan += [[6, tc["codec_bos_id"], 0, b, ni + 3 + np_ - 1]]
    plan += [[7 + i, -1, 1, b, i] for i in range(nt - 1)]
    plan += [[5, -1, 1, b, nt - 1]]
    return text, plan, ni + 3 + np_, nt
