"""Python (ctypes) binding of the MI355X drop-in library lib/libqwen_tts_amd.so.

This is the binding a maintainer of the reference would add next to its CLI
(see INTEGRATION.md): it mirrors `qwen_tts.h` (ctx struct + functions) and
`qtts_hip.h` (kernel-level entry points on device buffers).  Tests and
bench.py use it; device buffers for the kernel-level calls are torch tensors
(PyTorch is plumbing only: allocation, streams, torch.distributed).

The library is required: importing works without a GPU (symbols resolve),
but every compute call needs the HIP device and fails loudly without it.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# QTTS_LIB: another build of the same library (A/B measurements of two builds
# in one process tree); the default is the in-tree build
LIB_PATH = os.environ.get("QTTS_LIB") or os.path.join(HERE, "lib", "libqwen_tts_amd.so")
CLI_PATH = os.path.join(HERE, "bin", "qwen-tts")

_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)

PROGRESS_CB = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_void_p)
QUEUE_NEXT_CB = C.CFUNCTYPE(C.c_int, C.c_void_p)
AUDIO_CB = C.CFUNCTYPE(None, C.POINTER(C.c_float), C.c_int, C.c_void_p)
BATCH_AUDIO_CB = C.CFUNCTYPE(None, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p)
TEXT_FEED_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p)   # qwen_tts_text_feed_cb(feed, wait, userdata)


class Config(C.Structure):  # qwen_tts_config_t (include/qwen_tts.h)
    _fields_ = [(n, C.c_int) for n in (
        "talker_vocab_size", "talker_hidden", "talker_intermediate", "talker_layers", "talker_heads",
        "talker_kv_heads", "talker_head_dim", "talker_text_hidden", "talker_text_vocab", "num_code_groups")] + [
        ("talker_rms_norm_eps", C.c_float), ("talker_rope_theta", C.c_float), ("mrope_section", C.c_int * 3)] + [
        (n, C.c_int) for n in (
            "subtalker_vocab_size", "subtalker_hidden", "subtalker_intermediate", "subtalker_layers",
            "subtalker_heads", "subtalker_kv_heads", "subtalker_head_dim",
            "codec_num_quantizers", "codec_codebook_size", "codec_codebook_dim", "codec_hidden", "codec_latent",
            "codec_layers", "codec_heads", "codec_kv_heads", "codec_intermediate", "codec_sliding_window",
            "codec_decoder_dim")] + [
        ("codec_rms_norm_eps", C.c_float), ("codec_layer_scale", C.c_float),
        ("codec_upsample_rates", C.c_int * 4), ("codec_upsampling_ratios", C.c_int * 2),
        ("n_speakers", C.c_int), ("speaker_names", C.POINTER(C.c_char_p)), ("speaker_ids", _ip),
        ("n_languages", C.c_int), ("language_names", C.POINTER(C.c_char_p)), ("language_ids", _ip)] + [
        (n, C.c_int) for n in ("codec_pad_id", "codec_bos_id", "codec_eos_id", "codec_nothink_id", "codec_think_id",
                               "codec_think_bos_id", "codec_think_eos_id")]


class Ctx(C.Structure):  # qwen_tts_ctx_t (include/qwen_tts.h)
    _fields_ = [
        ("config", Config), ("model_dir", C.c_char * 512), ("hip", C.c_void_p), ("hip_device", C.c_int),
        ("talker_kv_len", C.c_int), ("tk_x", _fp),
        ("temperature", C.c_float), ("subtalker_temperature", C.c_float), ("top_k", C.c_int),
        ("subtalker_top_k", C.c_int), ("top_p", C.c_float), ("subtalker_top_p", C.c_float),
        ("repetition_penalty", C.c_float), ("max_new_tokens", C.c_int), ("fixed_codec_tokens", C.c_int),
        ("sample_seed", C.c_int), ("progress_cb", C.c_void_p), ("progress_cb_userdata", C.c_void_p),
        ("perf_total_ms", C.c_double), ("perf_talker_ms", C.c_double), ("perf_codec_ms", C.c_double),
        ("perf_codec_tokens", C.c_int), ("perf_prefill_ms", C.c_double), ("perf_first_frame_ms", C.c_double),
        ("last_codes", _ip), ("last_frames", C.c_int), ("last_stop_reason", C.c_int), ("last_stop_step", C.c_int),
        ("perf_first_packet_ms", C.c_double),
        ("tokenizer", C.c_void_p),
        ("queue_n", C.c_int), ("queue_codes", C.POINTER(_ip)), ("queue_frames", _ip), ("queue_stop_reason", _ip),
        ("queue_slot", _ip), ("queue_slots", C.c_int), ("queue_frames_launched", C.c_int),
        ("queue_refills", C.c_int), ("queue_slot_frames_used", C.c_longlong), ("queue_rows_launched", C.c_longlong),
        ("instruct", C.c_void_p), ("sampling", C.c_void_p), ("force", C.c_void_p),
    ]


class Sampling(C.Structure):  # qwen_tts_sampling_t (include/qwen_tts.h)
    _fields_ = [("temperature", C.c_float), ("top_p", C.c_float), ("repetition_penalty", C.c_float),
                ("top_k", C.c_int), ("subtalker_temperature", C.c_float), ("subtalker_top_p", C.c_float),
                ("subtalker_top_k", C.c_int), ("sample_seed", C.c_int)]


class SlotParams(C.Structure):  # qtts_slot_params_t (include/qtts_hip.h)
    _fields_ = [("temperature", C.c_float), ("top_p", C.c_float), ("repetition_penalty", C.c_float),
                ("top_k", C.c_int), ("st_temperature", C.c_float), ("st_top_p", C.c_float), ("st_top_k", C.c_int),
                ("seed", C.c_int)]


# Every symbol include/qwen_tts.h and include/qtts_hip.h declare (checked by tests/test_host.py)
EXPORTS = [
    "qwen_tts_load", "qwen_tts_free", "qwen_tts_set_progress_callback", "qwen_tts_generate", "qwen_tts_write_wav",
    "qwen_tts_talker_prefill", "qwen_tts_talker_forward", "qwen_tts_subtalker_generate", "qwen_tts_codec_decode",
    "qwen_tts_talker_hidden", "qwen_tts_load_on", "qwen_tts_generate_batch", "qwen_tts_last_codes", "qwen_tts_last_codes_slot",
    "qwen_tts_abi_sizeof_ctx", "qwen_tts_verbose", "qwen_tts_generate_stream", "qwen_tts_codec_stream_begin",
    "qwen_tts_codec_stream_push", "qwen_tts_generate_voice_clone",
    "qwen_tts_generate_voice_clone_batch", "qwen_tts_generate_voice_clone_stream", "qwen_tts_tokenize",
    "qwen_tts_text_prompt", "qwen_tts_speaker_embedding", "qwen_tts_encode_audio",
    "qwen_tts_generate_voice_clone_audio", "qwen_tts_generate_voice_clone_audio_batch",
    "qwen_tts_generate_voice_clone_audio_stream", "qtts_dev_codec_timing", "qtts_dev_codec_stage_ms", "qwen_tts_resample",
    "qtts_hip_device_count", "qtts_dev_create", "qtts_dev_destroy", "qtts_dev_put_tensor", "qtts_dev_finalize",
    "qtts_dev_bytes", "qtts_dev_begin", "qtts_dev_prompt", "qtts_dev_prompt_ref", "qtts_dev_prefill", "qtts_dev_frame", "qtts_dev_poll", "qtts_dev_frame_done",
    "qtts_dev_get_codes", "qtts_dev_codec_slot", "qtts_dev_talker_prefill_host", "qtts_dev_talker_forward_host",
    "qtts_dev_subtalker_host", "qtts_dev_codec_decode_host", "qtts_hip_matvec_bf16",
    "qtts_hip_rmsnorm_matvec_bf16", "qtts_hip_decode_matvec_bf16", "qtts_hip_resident_matvec_bf16", "qtts_hip_sample_top_k", "qtts_hip_causal_conv1d",
    "qtts_hip_transposed_conv1d", "qtts_hip_snake_beta", "qtts_hip_expf_glibc", "qtts_hip_sync",
    "qtts_dev_profile_frame", "qtts_hip_hbm_bw", "qtts_dev_codec_stream_begin", "qtts_dev_codec_stream_begin_ex",
    "qtts_dev_codec_stream_prime", "qtts_dev_codec_stream_push_slot",
    "qtts_dev_codec_stream_push_host", "qtts_dev_codec_async_begin", "qtts_dev_codec_async_push",
    "qtts_dev_codec_async_end", "qtts_dev_codec_multi", "qtts_dev_enc_config", "qtts_dev_enc_available", "qtts_dev_speaker_embed",
    "qtts_dev_encode_audio", "qwen_tts_generate_queue", "qwen_tts_queue_codes", "qtts_dev_reserve", "qtts_dev_refill",
    "qtts_dev_retire", "qtts_dev_frame_stops", "qtts_dev_move_slot", "qtts_dev_set_rows",
    "qwen_tts_set_kv_cache_dtype", "qwen_tts_kv_cache_dtype", "qtts_dev_set_kv_dtype", "qtts_dev_kv_dtype",
    "qtts_dev_get_kv", "qtts_dev_get_attn", "qtts_hip_attn_decode",
    "qtts_hip_attn_decode_ex", "qtts_hip_attn_cached", "qtts_hip_attn_o",
    "qtts_hip_attn_o_pair", "qtts_hip_resident_matvec_rows_bf16", "qtts_hip_st_pair_passes",
    "qwen_tts_force_codes", "qwen_tts_tap_draw", "qwen_tts_last_drawn", "qwen_tts_tap_result",
    "qtts_dev_force", "qtts_dev_tap", "qtts_dev_get_drawn", "qtts_dev_get_tap",
    "qtts_hip_xgemm_plan", "qtts_hip_xgemm_case", "qtts_hip_xgemm_func",
    "qtts_hip_batch_matvec_case", "qtts_hip_gemv_wide_launches", "qtts_hip_batch_matvec_plan",
    "qwen_tts_sampling_defaults", "qwen_tts_set_utterance_sampling", "qtts_dev_slot_params",
    "qtts_hip_sample_slot_launches", "qtts_hip_sample_top_k_rows",
    "qtts_hip_sample_nucleus", "qtts_hip_sample_nucleus_rows",
    "qwen_tts_generate_batch_stream", "qwen_tts_codec_mstream_begin", "qwen_tts_codec_mstream_push",
    "qtts_dev_codec_mstream_begin", "qtts_dev_codec_mstream_push_slots", "qtts_dev_codec_mstream_push_host",
    "qtts_dev_codec_mstream_pos", "qtts_hip_xgemm_seg_case",
    "qwen_tts_generate_queue_stream", "qwen_tts_codec_mstream_push_any", "qwen_tts_codec_mstream_reset",
    "qtts_dev_codec_mstream_push_host_any", "qtts_dev_codec_mstream_push_slots_at", "qtts_dev_codec_mstream_reset",
    "qwen_tts_codec_mstream_push_ragged", "qtts_dev_codec_mstream_push_host_ragged",
    "qtts_dev_codec_mstream_push_slots_ragged", "qtts_dev_codec_mstream_prime",
    "qwen_tts_generate_voice_clone_batch_stream", "qwen_tts_generate_voice_clone_audio_batch_stream",
    "qtts_dev_codec_mstream_save", "qtts_dev_codec_mstream_restore", "qtts_dev_codec_snapshot_free",
    "qtts_dev_codec_snapshot_pos", "qtts_dev_codec_snapshot_bytes",
    "qwen_tts_codec_mstream_save", "qwen_tts_codec_mstream_restore", "qwen_tts_codec_snapshot_free",
    "qwen_tts_codec_snapshot_pos", "qwen_tts_voice_create", "qwen_tts_voice_create_audio", "qwen_tts_voice_info",
    "qwen_tts_voice_free", "qwen_tts_generate_voice_queue", "qwen_tts_generate_voice_queue_stream",
    "qwen_tts_set_utterance_instruct", "qwen_tts_instruct_prompt", "qtts_dev_prefix_cache",
    "qtts_dev_prefix_cache_bytes", "qtts_hip_prefix_hits", "qtts_hip_prefix_misses", "qtts_hip_prefill_rows",
    "qtts_dev_get_hidden",
    "qwen_tts_feed_ids", "qwen_tts_feed_close", "qwen_tts_feed_state", "qwen_tts_generate_fed_stream",
    "qwen_tts_generate_fed_batch_stream", "qtts_dev_text_open", "qtts_dev_text_append", "qtts_dev_get_trailing",
    "qtts_dev_text_state", "qtts_hip_text_held_frames", "qtts_dev_text_append_ms",
    "qtts_hip_rows_gemm_plan", "qtts_hip_rows_gemm_case",
    "qtts_hip_econv_plan", "qtts_hip_econv_case", "qtts_hip_enc_op", "qtts_hip_enc_func",
]

MAX_BATCH = 64   # QWEN_TTS_MAX_BATCH / QTTS_HIP_MAX_BATCH: lock-step slots per context


class FeedHandle:
    """The feed a text callback pushes into (qwen_tts_feed_t; valid inside the callback only)."""

    def __init__(self, ptr):
        self._p = C.c_void_p(ptr)

    def push(self, utterance, ids):
        """content ids of `utterance`, any number >= 1; 0, or -1 where the library refuses"""
        a = np.ascontiguousarray(ids, np.int32)
        return int(lib().qwen_tts_feed_ids(self._p, int(utterance), a.ctypes.data_as(_ip), int(a.size)))

    def close(self, utterance):
        """the utterance's text is over (the tts_eos row); 0 or -1"""
        return int(lib().qwen_tts_feed_close(self._p, int(utterance)))

    def state(self, utterance):
        """(ids taken, frames launched, starved) or None for a bad index"""
        t, f, s = C.c_int(0), C.c_int(0), C.c_int(0)
        if lib().qwen_tts_feed_state(self._p, int(utterance), C.byref(t), C.byref(f), C.byref(s)) != 0:
            return None
        return t.value, f.value, bool(s.value)


class BGemvDesc(C.Structure):
    """qtts_bgemv_desc_t (include/qtts_hip.h): one lock-step batch decode GEMV;
    the pointers are device addresses."""
    _fields_ = [
        ("rows", C.c_int), ("cols", C.c_int), ("batch", C.c_int),
        ("A", C.c_void_p),
        ("src", C.c_int),
        ("x", C.c_void_p), ("ldx", C.c_int),
        ("table", C.c_void_p),
        ("ids", C.c_void_p), ("ids_bstride", C.c_int), ("ids_rstride", C.c_int), ("ids_off", C.c_int),
        ("row_sel", C.c_void_p),
        ("part_in", C.c_void_p), ("n_part_in", C.c_int),
        ("norm_w", C.c_void_p), ("eps", C.c_float),
        ("xcopy", C.c_void_p), ("xcopy_normed", C.c_int),
        ("epi", C.c_int),
        ("bias", C.c_void_p),
        ("y", C.c_void_p), ("ldy", C.c_int),
        ("kz", C.c_int), ("self_reduce", C.c_int),
        ("part_out", C.c_void_p),
    ]


class BGemvPlan(C.Structure):
    """qtts_bgemv_plan_t (include/qtts_hip.h): the batch GEMV planner's answer."""
    _fields_ = [
        ("kernel", C.c_int),
        ("n_tmpl", C.c_int), ("tmpl", C.c_int * 5),
        ("src", C.c_int),
        ("grid_x", C.c_int), ("grid_y", C.c_int), ("block", C.c_int),
        ("lds_bytes", C.c_size_t),
        ("tpw", C.c_int), ("cch", C.c_int),
    ]


BGEMV_KERNELS = {1: "k_gemvm", 2: "k_gemvb", 4: "k_gemvx"}   # qtts_bgemv_plan_t.kernel


class RowsGemmDesc(C.Structure):
    """qtts_rows_gemm_desc_t (include/qtts_hip.h): one multi-row projection of
    the prefill and prompt paths; the pointers are device addresses."""
    _fields_ = [
        ("rows", C.c_int), ("R", C.c_int), ("C", C.c_int),
        ("A", C.c_void_p),
        ("src", C.c_int),
        ("x", C.c_void_p), ("ldx", C.c_int),
        ("table", C.c_void_p),
        ("ids", C.c_void_p), ("ids_bstride", C.c_int),
        ("norm_w", C.c_void_p), ("eps", C.c_float),
        ("epi", C.c_int),
        ("bias", C.c_void_p),
        ("y", C.c_void_p), ("ldy", C.c_int),
        ("part", C.c_void_p), ("part_elems", C.c_size_t),
        ("planes", C.c_void_p), ("plane_elems", C.c_size_t),
        ("inv", C.c_void_p),
    ]


class RowsGemmPlan(C.Structure):
    """qtts_rows_gemm_plan_t (include/qtts_hip.h): what the multi-row GEMMs launch."""
    _fields_ = [
        ("kernel", C.c_int), ("kz", C.c_int),
        ("grid_x", C.c_int), ("grid_y", C.c_int), ("grid_z", C.c_int), ("block", C.c_int),
    ]


# qtts_rows_gemm_plan_t.kernel (QTTS_RG_* of qtts_hip.h)
RG_NAMES = ["k_mgemm<1,1>", "k_mgemm<2,1>", "k_mgemm<4,1>", "k_mgemm<4,2>", "k_mgemm<4,4>", "k_pgemm<2>", "k_pgemm<4>"]


class EConvDesc(C.Structure):
    """qtts_econv_desc_t (include/qtts_hip.h): one launch of the voice-clone
    encoders' contraction kernel k_econv, as the encoders describe it.  Device
    pointers as integers; w is fp32 [M][ci * kw]."""
    _fields_ = [("M", C.c_int), ("ci", C.c_int), ("kw", C.c_int), ("stride", C.c_int), ("dil", C.c_int),
                ("padl", C.c_int), ("pmode", C.c_int), ("act_in", C.c_int),
                ("w", C.c_void_p),
                ("x", C.c_void_p), ("x2", C.c_void_p), ("xb", C.c_size_t), ("xc", C.c_int), ("xt", C.c_int),
                ("lin", C.c_int * 16), ("lout", C.c_int * 16), ("nb", C.c_int), ("nmax", C.c_int),
                ("y", C.c_void_p), ("yb", C.c_size_t), ("yc", C.c_int), ("yt", C.c_int),
                ("bias", C.c_void_p), ("bias2", C.c_void_p), ("bias2_b", C.c_int), ("act_out", C.c_int),
                ("vec", C.c_void_p),
                ("res", C.c_void_p), ("rb", C.c_size_t), ("rc", C.c_int), ("rt", C.c_int),
                ("part", C.c_void_p), ("part_elems", C.c_size_t)]


class EConvPlan(C.Structure):
    """qtts_econv_plan_t (include/qtts_hip.h): what launch_econv launches."""
    _fields_ = [("rows", C.c_int), ("kz", C.c_int), ("grid_x", C.c_int), ("grid_y", C.c_int), ("grid_z", C.c_int),
                ("part_elems", C.c_size_t)]


class EncOp(C.Structure):
    """qtts_enc_op_t (include/qtts_hip.h): one launch of one small encoder kernel."""
    _fields_ = [("op", C.c_int), ("inp", C.c_void_p * 6), ("out", C.c_void_p * 2), ("n", C.c_int * 8),
                ("s", C.c_size_t * 3), ("eps", C.c_float)]


# qtts_enc_op_t.op (QTTS_EO_* of qtts_hip.h)
(EO_MEL, EO_ROW_MEAN, EO_EGEMV, EO_SE_APPLY, EO_ASP_STATS, EO_ASP_POOL, EO_LN_ROWS, EO_ROPE_BT, EO_ROWS_BT,
 EO_RVQ_ENC) = range(10)
# k_econv padding modes and activations (k_enc.hip)
EPAD_ZERO, EPAD_REFLECT, EPAD_REPLICATE = range(3)
EACT_NONE, EACT_RELU, EACT_RELU_TANH, EACT_GELU, EACT_SIGMOID = range(5)


class XGemmDesc(C.Structure):
    """qtts_xgemm_desc_t (include/qtts_hip.h): one contraction of the codec's
    GEMM family; the pointers are device addresses."""
    _fields_ = [
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("amode", C.c_int), ("bmode", C.c_int), ("emode", C.c_int),
        ("A", C.c_void_p), ("lda", C.c_int),
        ("B", C.c_void_p), ("ldb", C.c_int),
        ("Kw", C.c_int), ("dil", C.c_int), ("pad", C.c_int), ("L", C.c_int), ("stride", C.c_int),
        ("tmin", C.c_int), ("co", C.c_int),
        ("sa", C.c_void_p), ("sb", C.c_void_p),
        ("C", C.c_void_p), ("ldc", C.c_int),
        ("bias", C.c_void_p), ("vec", C.c_void_p), ("aux", C.c_void_p), ("res", C.c_void_p),
        ("ldaux", C.c_int), ("ldres", C.c_int),
        ("ea", C.c_void_p), ("eb", C.c_void_p),
    ]


# XGemm modes and kernels (qtts_codec.h, QTTS_XP_* of qtts_hip.h)
XA_ROWS, XA_TRANS, XA_TCONV_W = 0, 1, 2
XB_WT, XB_CONV, XB_TCONV = 0, 1, 2
(XE_STORE, XE_BIAS_N, XE_BIAS_N_GELU, XE_SILU_MUL, XE_SCALE_RESID_N, XE_BIAS_T, XE_BIAS_GAMMA_RES_T, XE_BIAS_M,
 XE_BIAS_M_RES, XE_BIAS_M_SNAKE) = range(10)
XP_CONVB2, XP_CONVB4, XP_CONV, XP_XLIN, XP_XGEMV, XP_XGEMM = range(6)
XP_NAMES = ["k_convb<Kw,2>", "k_convb<Kw,4>", "k_conv<Kw>", "k_xlin", "k_xgemv", "k_xgemm"]

MAX_TAPS = 8   # taps per run (qwen_tts_tap_draw)

KV_F32, KV_BF16 = 0, 1   # QWEN_TTS_KV_F32 / QWEN_TTS_KV_BF16

_LIB = None


def tokenize(model_dir, text):
    """Qwen2 BPE ids of `text` (qwen_tts_tokenize: the model dir's vocab.json /
    merges.txt; no GPU needed).  None on error."""
    n = C.c_int(0)
    p = lib().qwen_tts_tokenize(model_dir.encode(), text.encode("utf-8"), C.byref(n))
    if not p:
        return None
    ids = np.ctypeslib.as_array(C.cast(p, _ip), shape=(n.value,)).tolist() if n.value else []
    _libc.free(C.c_void_p(p))
    return ids


def resample(wav, sr_in, sr_out=24000):
    """qwen_tts_resample (host C, no GPU needed): librosa's polyphase method =
    scipy.signal.resample_poly."""
    w = np.ascontiguousarray(wav, np.float32)
    n = C.c_int(0)
    p = lib().qwen_tts_resample(w.ctypes.data_as(_fp), w.shape[0], int(sr_in), int(sr_out), C.byref(n))
    if not p:
        return None
    out = np.ctypeslib.as_array(C.cast(p, _fp), shape=(n.value,)).copy()
    _libc.free(C.c_void_p(p))
    return out


def lib():
    """Load the in-tree library (raises if it was not built)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # torch bundles its own HIP runtime with the same soname (libamdhip64.so.7)
    # as /opt/rocm's.  Loading torch first makes this library bind to that one
    # runtime, so torch tensors, streams and our launches share it; loading
    # ours first would put two HIP runtimes in the process and break torch.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} missing: run `make -C qwen3-tts-c_amd` (or __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    L.qwen_tts_load.restype = C.POINTER(Ctx)
    L.qwen_tts_load.argtypes = [C.c_char_p]
    L.qwen_tts_free.argtypes = [C.POINTER(Ctx)]
    L.qwen_tts_generate.restype = C.c_void_p
    L.qwen_tts_generate.argtypes = [C.POINTER(Ctx), C.c_char_p, C.c_char_p, C.c_char_p, _ip]
    L.qwen_tts_generate_batch.restype = C.c_int
    L.qwen_tts_generate_batch.argtypes = [C.POINTER(Ctx), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                          C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), _ip]
    L.qwen_tts_last_codes.restype = C.c_int
    L.qwen_tts_last_codes.argtypes = [C.POINTER(Ctx), _ip, C.c_int]
    L.qwen_tts_last_codes_slot.restype = C.c_int
    L.qwen_tts_last_codes_slot.argtypes = [C.POINTER(Ctx), C.c_int, _ip, C.c_int]
    L.qwen_tts_generate_queue.restype = C.c_int
    L.qwen_tts_generate_queue.argtypes = [C.POINTER(Ctx), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                          C.POINTER(C.c_char_p), C.c_int, QUEUE_NEXT_CB, C.c_void_p,
                                          C.POINTER(C.c_void_p), _ip]
    L.qwen_tts_queue_codes.restype = C.c_int
    L.qwen_tts_queue_codes.argtypes = [C.POINTER(Ctx), C.c_int, _ip, C.c_int]
    L.qwen_tts_talker_prefill.argtypes = [C.POINTER(Ctx), _fp, C.c_int]
    L.qwen_tts_talker_forward.argtypes = [C.POINTER(Ctx), _fp, _fp]
    L.qwen_tts_subtalker_generate.argtypes = [C.POINTER(Ctx), _fp, C.c_int, _ip]
    L.qwen_tts_codec_decode.restype = C.c_void_p
    L.qwen_tts_codec_decode.argtypes = [C.POINTER(Ctx), _ip, C.c_int, _ip]
    L.qwen_tts_talker_hidden.argtypes = [C.POINTER(Ctx), _fp]
    L.qwen_tts_load_on.restype = C.POINTER(Ctx)
    L.qwen_tts_load_on.argtypes = [C.c_char_p, C.c_int]
    L.qwen_tts_set_progress_callback.argtypes = [C.POINTER(Ctx), PROGRESS_CB, C.c_void_p]
    L.qwen_tts_write_wav.argtypes = [C.c_char_p, _fp, C.c_int, C.c_int]
    L.qwen_tts_abi_sizeof_ctx.restype = C.c_size_t
    L.qwen_tts_resample.restype = C.c_void_p
    L.qwen_tts_resample.argtypes = [_fp, C.c_int, C.c_int, C.c_int, _ip]
    L.qwen_tts_tokenize.restype = C.c_void_p
    L.qwen_tts_tokenize.argtypes = [C.c_char_p, C.c_char_p, _ip]
    L.qwen_tts_text_prompt.restype = C.c_void_p
    L.qwen_tts_text_prompt.argtypes = [C.POINTER(Ctx), C.c_char_p]
    L.qwen_tts_generate_stream.restype = C.c_void_p
    L.qwen_tts_generate_stream.argtypes = [C.POINTER(Ctx), C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, AUDIO_CB,
                                           C.c_void_p, _ip]
    L.qwen_tts_generate_voice_clone_stream.restype = C.c_void_p
    L.qwen_tts_generate_voice_clone_stream.argtypes = [C.POINTER(Ctx), C.c_char_p, C.c_char_p, _ip, C.c_int, _fp,
                                                       C.c_char_p, C.c_int, C.c_int, AUDIO_CB, C.c_void_p, _ip]
    L.qwen_tts_generate_voice_clone.restype = C.c_void_p
    L.qwen_tts_generate_voice_clone.argtypes = [C.POINTER(Ctx), C.c_char_p, C.c_char_p, _ip, C.c_int, _fp,
                                                C.c_char_p, C.c_int, _ip]
    L.qwen_tts_generate_voice_clone_batch.restype = C.c_int
    L.qwen_tts_generate_voice_clone_batch.argtypes = [C.POINTER(Ctx), C.c_int, C.POINTER(C.c_char_p),
                                                      C.POINTER(C.c_char_p), C.POINTER(_ip), _ip, C.POINTER(_fp),
                                                      C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_void_p), _ip]
    L.qwen_tts_codec_stream_begin.argtypes = [C.POINTER(Ctx), C.c_int]
    L.qwen_tts_codec_stream_push.argtypes = [C.POINTER(Ctx), _ip, C.c_int, _fp]
    # (an older build named by QTTS_LIB for a same-box A/B has no multi-stream entries; build() checks EXPORTS)
    if hasattr(L, "qwen_tts_generate_fed_batch_stream"):   # (an older build named by QTTS_LIB has no fed entries)
        L.qwen_tts_feed_ids.restype = C.c_int
        L.qwen_tts_feed_ids.argtypes = [C.c_void_p, C.c_int, _ip, C.c_int]
        L.qwen_tts_feed_close.restype = C.c_int
        L.qwen_tts_feed_close.argtypes = [C.c_void_p, C.c_int]
        L.qwen_tts_feed_state.restype = C.c_int
        L.qwen_tts_feed_state.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _ip]
        L.qwen_tts_generate_fed_stream.restype = C.c_void_p
        L.qwen_tts_generate_fed_stream.argtypes = [C.POINTER(Ctx), C.c_char_p, C.c_char_p, C.c_int, TEXT_FEED_CB,
                                                   C.c_void_p, AUDIO_CB, C.c_void_p, _ip]
        L.qwen_tts_generate_fed_batch_stream.restype = C.c_int
        L.qwen_tts_generate_fed_batch_stream.argtypes = [C.POINTER(Ctx), C.c_int, C.POINTER(C.c_char_p),
                                                         C.POINTER(C.c_char_p), C.c_int, TEXT_FEED_CB, C.c_void_p,
                                                         BATCH_AUDIO_CB, C.c_void_p, C.POINTER(C.c_void_p), _ip]
        L.qtts_dev_text_open.restype = C.c_int
        L.qtts_dev_text_open.argtypes = [C.c_void_p, C.c_int]
        L.qtts_dev_text_append.restype = C.c_int
        L.qtts_dev_text_append.argtypes = [C.c_void_p, C.c_int, _ip, C.c_int, C.c_int]
        L.qtts_dev_text_append_ms.restype = C.c_int
        L.qtts_dev_text_append_ms.argtypes = [C.c_void_p, C.c_int, _ip, C.c_int, C.c_int, _fp]
        L.qtts_dev_get_trailing.restype = C.c_int
        L.qtts_dev_get_trailing.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _fp]
        L.qtts_dev_text_state.restype = C.c_int
        L.qtts_dev_text_state.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _ip]
        L.qtts_hip_text_held_frames.restype = C.c_longlong
        L.qtts_hip_text_held_frames.argtypes = []
    if hasattr(L, "qwen_tts_generate_batch_stream"):
        L.qwen_tts_generate_batch_stream.argtypes = [C.POINTER(Ctx), C.c_int, C.POINTER(C.c_char_p),
                                                     C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int,
                                                     BATCH_AUDIO_CB, C.c_void_p, C.POINTER(C.c_void_p), _ip]
        L.qwen_tts_codec_mstream_begin.argtypes = [C.POINTER(Ctx), C.c_int, C.c_int]
        L.qwen_tts_codec_mstream_push.argtypes = [C.POINTER(Ctx), C.c_int, _ip, _ip, C.c_int, C.POINTER(_fp)]
        L.qtts_dev_codec_mstream_begin.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.qtts_dev_codec_mstream_push_slots.argtypes = [C.c_void_p, C.c_int, _ip, _ip, C.c_int, C.c_int,
                                                        C.POINTER(_fp)]
        L.qtts_dev_codec_mstream_push_host.argtypes = [C.c_void_p, C.c_int, _ip, _ip, C.c_int, C.POINTER(_fp)]
        L.qtts_dev_codec_mstream_pos.argtypes = [C.c_void_p, C.c_int]
        L.qtts_hip_xgemm_seg_case.restype = C.c_int
        L.qtts_hip_xgemm_seg_case.argtypes = [C.POINTER(XGemmDesc), C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int,
                                              _ip, _ip, C.c_void_p]
    # (nor the streaming queue's)
    if hasattr(L, "qwen_tts_generate_queue_stream"):
        L.qwen_tts_generate_queue_stream.restype = C.c_int
        L.qwen_tts_generate_queue_stream.argtypes = [C.POINTER(Ctx), C.c_int, C.POINTER(C.c_char_p),
                                                     C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int,
                                                     QUEUE_NEXT_CB, C.c_void_p, C.c_int, BATCH_AUDIO_CB, C.c_void_p,
                                                     C.POINTER(C.c_void_p), _ip]
        L.qwen_tts_codec_mstream_push_any.argtypes = [C.POINTER(Ctx), C.c_int, _ip, _ip, C.c_int, C.POINTER(_fp)]
        L.qwen_tts_codec_mstream_reset.argtypes = [C.POINTER(Ctx), C.c_int]
        L.qtts_dev_codec_mstream_push_host_any.argtypes = [C.c_void_p, C.c_int, _ip, _ip, C.c_int, C.POINTER(_fp)]
        L.qtts_dev_codec_mstream_push_slots_at.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _ip, C.c_int,
                                                           C.POINTER(_fp)]
        L.qtts_dev_codec_mstream_reset.argtypes = [C.c_void_p, C.c_int]
    # (nor the ragged pushes)
    if hasattr(L, "qwen_tts_codec_mstream_push_ragged"):
        L.qwen_tts_codec_mstream_push_ragged.argtypes = [C.POINTER(Ctx), C.c_int, _ip, _ip, _ip, C.c_int,
                                                         C.POINTER(_fp)]
        L.qtts_dev_codec_mstream_push_host_ragged.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _ip, C.c_int,
                                                              C.POINTER(_fp)]
        L.qtts_dev_codec_mstream_push_slots_ragged.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _ip, _ip,
                                                               C.POINTER(_fp)]
        L.qtts_dev_codec_mstream_prime.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _ip, C.c_int]
        L.qwen_tts_generate_voice_clone_batch_stream.restype = C.c_int
        L.qwen_tts_generate_voice_clone_batch_stream.argtypes = [
            C.POINTER(Ctx), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(_ip), _ip,
            C.POINTER(_fp), C.POINTER(C.c_char_p), C.c_int, C.c_int, BATCH_AUDIO_CB, C.c_void_p,
            C.POINTER(C.c_void_p), _ip]
        L.qwen_tts_generate_voice_clone_audio_batch_stream.restype = C.c_int
        L.qwen_tts_generate_voice_clone_audio_batch_stream.argtypes = [
            C.POINTER(Ctx), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(_fp), _ip,
            C.POINTER(C.c_char_p), _ip, C.c_int, C.c_int, BATCH_AUDIO_CB, C.c_void_p, C.POINTER(C.c_void_p), _ip]
    # (nor the codec snapshots, the voice handles and the voice queue)
    if hasattr(L, "qwen_tts_voice_create"):
        L.qtts_dev_codec_mstream_save.restype = C.c_void_p
        L.qtts_dev_codec_mstream_save.argtypes = [C.c_void_p, C.c_int]
        L.qtts_dev_codec_mstream_restore.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.qtts_dev_codec_snapshot_free.restype = None
        L.qtts_dev_codec_snapshot_free.argtypes = [C.c_void_p]
        L.qtts_dev_codec_snapshot_pos.argtypes = [C.c_void_p]
        L.qtts_dev_codec_snapshot_bytes.restype = C.c_longlong
        L.qtts_dev_codec_snapshot_bytes.argtypes = [C.c_void_p]
        L.qwen_tts_codec_mstream_save.restype = C.c_void_p
        L.qwen_tts_codec_mstream_save.argtypes = [C.POINTER(Ctx), C.c_int]
        L.qwen_tts_codec_mstream_restore.argtypes = [C.POINTER(Ctx), C.c_int, C.c_void_p]
        L.qwen_tts_codec_snapshot_free.restype = None
        L.qwen_tts_codec_snapshot_free.argtypes = [C.c_void_p]
        L.qwen_tts_codec_snapshot_pos.argtypes = [C.c_void_p]
        L.qwen_tts_voice_create.restype = C.c_void_p
        L.qwen_tts_voice_create.argtypes = [C.POINTER(Ctx), C.c_char_p, _ip, C.c_int, _fp]
        L.qwen_tts_voice_create_audio.restype = C.c_void_p
        L.qwen_tts_voice_create_audio.argtypes = [C.POINTER(Ctx), C.c_char_p, _fp, C.c_int, C.c_int]
        L.qwen_tts_voice_info.argtypes = [C.c_void_p, _ip, _ip]
        L.qwen_tts_voice_free.restype = None
        L.qwen_tts_voice_free.argtypes = [C.c_void_p]
        L.qwen_tts_generate_voice_queue.restype = C.c_int
        L.qwen_tts_generate_voice_queue.argtypes = [C.POINTER(Ctx), C.c_int, C.POINTER(C.c_char_p),
                                                    C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                                    QUEUE_NEXT_CB, C.c_void_p, C.POINTER(C.c_void_p), _ip]
        L.qwen_tts_generate_voice_queue_stream.restype = C.c_int
        L.qwen_tts_generate_voice_queue_stream.argtypes = [C.POINTER(Ctx), C.c_int, C.POINTER(C.c_char_p),
                                                           C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), C.c_int,
                                                           C.c_int, QUEUE_NEXT_CB, C.c_void_p, C.c_int, BATCH_AUDIO_CB,
                                                           C.c_void_p, C.POINTER(C.c_void_p), _ip]
    L.qwen_tts_speaker_embedding.restype = C.c_void_p
    L.qwen_tts_speaker_embedding.argtypes = [C.POINTER(Ctx), _fp, C.c_int, _ip]
    L.qwen_tts_encode_audio.restype = C.c_void_p
    L.qwen_tts_encode_audio.argtypes = [C.POINTER(Ctx), _fp, C.c_int, _ip]
    L.qwen_tts_generate_voice_clone_audio.restype = C.c_void_p
    L.qwen_tts_generate_voice_clone_audio.argtypes = [C.POINTER(Ctx), C.c_char_p, C.c_char_p, _fp, C.c_int,
                                                      C.c_char_p, C.c_int, C.c_int, _ip]
    L.qwen_tts_generate_voice_clone_audio_batch.restype = C.c_int
    L.qwen_tts_generate_voice_clone_audio_batch.argtypes = [C.POINTER(Ctx), C.c_int, C.POINTER(C.c_char_p),
                                                            C.POINTER(C.c_char_p), C.POINTER(_fp), _ip,
                                                            C.POINTER(C.c_char_p), _ip, C.c_int,
                                                            C.POINTER(C.c_void_p), _ip]
    L.qwen_tts_generate_voice_clone_audio_stream.restype = C.c_void_p
    L.qwen_tts_generate_voice_clone_audio_stream.argtypes = [C.POINTER(Ctx), C.c_char_p, C.c_char_p, _fp, C.c_int,
                                                             C.c_char_p, C.c_int, C.c_int, C.c_int, AUDIO_CB,
                                                             C.c_void_p, _ip]
    L.qtts_dev_enc_available.restype = C.c_int
    L.qtts_dev_enc_available.argtypes = [C.c_void_p]
    L.qtts_dev_speaker_embed.restype = C.c_int
    L.qtts_dev_speaker_embed.argtypes = [C.c_void_p, C.c_int, C.POINTER(_fp), _ip, _fp, _fp]
    L.qtts_dev_encode_audio.restype = C.c_int
    L.qtts_dev_encode_audio.argtypes = [C.c_void_p, C.c_int, C.POINTER(_fp), _ip, _ip, C.c_int, _ip, _fp]
    L.qwen_tts_set_kv_cache_dtype.restype = C.c_int
    L.qwen_tts_set_kv_cache_dtype.argtypes = [C.POINTER(Ctx), C.c_int]
    L.qwen_tts_kv_cache_dtype.restype = C.c_int
    L.qwen_tts_kv_cache_dtype.argtypes = [C.POINTER(Ctx)]
    L.qtts_dev_set_kv_dtype.restype = C.c_int
    L.qtts_dev_set_kv_dtype.argtypes = [C.c_void_p, C.c_int]
    L.qtts_dev_kv_dtype.restype = C.c_int
    L.qtts_dev_kv_dtype.argtypes = [C.c_void_p]
    L.qtts_dev_get_kv.restype = C.c_int
    L.qtts_dev_get_kv.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp]
    L.qtts_dev_get_attn.restype = C.c_int
    L.qtts_dev_get_attn.argtypes = [C.c_void_p, _fp, _fp]
    L.qtts_dev_bytes.restype = C.c_size_t
    L.qtts_dev_bytes.argtypes = [C.c_void_p, C.c_int]
    _up = C.POINTER(C.c_uint)
    L.qwen_tts_force_codes.restype = C.c_int
    L.qwen_tts_force_codes.argtypes = [C.POINTER(Ctx), C.c_int, _ip, C.c_int]
    L.qwen_tts_tap_draw.restype = C.c_int
    L.qwen_tts_tap_draw.argtypes = [C.POINTER(Ctx), C.c_int, C.c_int, C.c_int]
    L.qwen_tts_last_drawn.restype = C.c_int
    L.qwen_tts_last_drawn.argtypes = [C.POINTER(Ctx), C.c_int, _ip, C.c_int]
    L.qwen_tts_tap_result.restype = C.c_int
    L.qwen_tts_tap_result.argtypes = [C.POINTER(Ctx), C.c_int, _fp, C.c_int, _up, _ip]
    L.qtts_dev_force.restype = C.c_int
    L.qtts_dev_force.argtypes = [C.c_void_p, C.c_int, _ip, C.c_int]
    L.qtts_dev_tap.restype = C.c_int
    L.qtts_dev_tap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.qtts_dev_get_drawn.restype = C.c_int
    L.qtts_dev_get_drawn.argtypes = [C.c_void_p, C.c_int, _ip, C.c_int]
    L.qtts_dev_get_tap.restype = C.c_int
    L.qtts_dev_get_tap.argtypes = [C.c_void_p, C.c_int, _fp, C.c_int, _up, _ip]
    L.qtts_hip_device_count.restype = C.c_int
    vp = C.c_void_p
    L.qtts_hip_matvec_bf16.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.qtts_hip_rmsnorm_matvec_bf16.argtypes = [vp, vp, vp, vp, C.c_float, C.c_int, C.c_int, C.c_int, vp]
    L.qtts_hip_decode_matvec_bf16.argtypes = [vp, vp, vp, vp, C.c_float, C.c_int, C.c_int, C.c_int, vp]
    L.qtts_hip_resident_matvec_bf16.argtypes = [vp, vp, vp, vp, C.c_float, C.c_int, C.c_int, C.c_int, vp]
    L.qtts_hip_sample_top_k.argtypes = [vp, vp, C.c_int, C.c_int, C.c_float, C.c_float, vp, C.c_int, vp]
    L.qtts_hip_causal_conv1d.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.qtts_hip_transposed_conv1d.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.qtts_hip_snake_beta.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp]
    L.qtts_hip_expf_glibc.argtypes = [vp, vp, C.c_int, vp]
    L.qtts_hip_attn_decode.restype = C.c_int
    L.qtts_hip_attn_decode.argtypes = [vp] * 9 + [C.c_int] * 5 + [C.c_float, C.c_int, vp]
    L.qtts_hip_attn_decode_ex.restype = C.c_int
    L.qtts_hip_attn_decode_ex.argtypes = [vp] * 9 + [C.c_int] * 5 + [C.c_float, C.c_int, vp, vp]
    L.qtts_hip_attn_cached.restype = C.c_int
    L.qtts_hip_attn_cached.argtypes = [vp, vp, C.c_int] + [vp] * 8 + [C.c_int] * 6 + [C.c_float] + [C.c_int] * 3 + [vp]
    L.qtts_hip_attn_o.restype = C.c_int
    L.qtts_hip_attn_o.argtypes = [vp] * 10 + [C.c_int] * 6 + [C.c_float, vp]
    # (an older build named by QTTS_LIB for a same-box A/B has no pair entries; build() checks EXPORTS)
    if hasattr(L, "qtts_hip_st_pair_passes"):
        L.qtts_hip_st_pair_passes.restype = C.c_longlong
        L.qtts_hip_attn_o_pair.restype = C.c_int
        L.qtts_hip_attn_o_pair.argtypes = [vp] * 10 + [C.c_int] * 5 + [C.c_float, vp]
        L.qtts_hip_resident_matvec_rows_bf16.restype = C.c_int
        L.qtts_hip_resident_matvec_rows_bf16.argtypes = ([vp] * 4 + [C.c_float] + [C.c_int] * 3 + [vp, C.c_int, vp,
                                                                                                C.c_int, vp])
    if hasattr(L, "qtts_hip_xgemm_case"):
        L.qtts_hip_xgemm_plan.restype = C.c_int
        L.qtts_hip_xgemm_plan.argtypes = [C.POINTER(XGemmDesc), C.c_size_t, C.c_int, _ip, _ip]
        L.qtts_hip_xgemm_case.restype = C.c_int
        L.qtts_hip_xgemm_case.argtypes = [C.POINTER(XGemmDesc), C.c_size_t, C.c_int, _ip, _ip, vp]
        L.qtts_hip_xgemm_func.restype = C.c_int
        L.qtts_hip_xgemm_func.argtypes = [vp] * 4 + [C.c_int] * 3 + [vp]
    if hasattr(L, "qtts_hip_batch_matvec_case"):
        L.qtts_hip_batch_matvec_case.restype = C.c_int
        L.qtts_hip_batch_matvec_case.argtypes = [C.POINTER(BGemvDesc), vp]
        L.qtts_hip_gemv_wide_launches.restype = C.c_longlong
        L.qtts_hip_gemv_wide_launches.argtypes = []
    if hasattr(L, "qtts_dev_slot_params"):
        L.qwen_tts_sampling_defaults.restype = C.c_int
        L.qwen_tts_sampling_defaults.argtypes = [C.POINTER(Ctx), C.POINTER(Sampling)]
        L.qwen_tts_set_utterance_sampling.restype = C.c_int
        L.qwen_tts_set_utterance_sampling.argtypes = [C.POINTER(Ctx), C.c_int, C.POINTER(Sampling)]
        L.qtts_dev_slot_params.restype = C.c_int
        L.qtts_dev_slot_params.argtypes = [C.c_void_p, C.c_int, C.POINTER(SlotParams)]
        L.qtts_hip_sample_slot_launches.restype = C.c_longlong
        L.qtts_hip_sample_slot_launches.argtypes = []
        L.qtts_hip_sample_top_k_rows.restype = C.c_int
        L.qtts_hip_sample_top_k_rows.argtypes = [vp, vp, C.c_int, _ip, _fp, _fp, vp, C.c_int, vp]
    if hasattr(L, "qtts_hip_sample_nucleus_rows"):
        L.qtts_hip_sample_nucleus.restype = C.c_int
        L.qtts_hip_sample_nucleus.argtypes = [vp, vp, C.c_int, C.c_int, C.c_float, C.c_float, vp, C.c_int, vp, vp]
        L.qtts_hip_sample_nucleus_rows.restype = C.c_int
        L.qtts_hip_sample_nucleus_rows.argtypes = [vp, vp, vp, C.c_int, _ip, _fp, _fp, vp, C.c_int, C.c_int, C.c_int,
                                                   vp]
    if hasattr(L, "qwen_tts_set_utterance_instruct"):
        L.qwen_tts_set_utterance_instruct.restype = C.c_int
        L.qwen_tts_set_utterance_instruct.argtypes = [C.POINTER(Ctx), C.c_int, C.POINTER(C.c_char_p)]
        L.qwen_tts_instruct_prompt.restype = C.c_void_p
        L.qwen_tts_instruct_prompt.argtypes = [C.POINTER(Ctx), C.c_char_p]
        L.qtts_dev_prefix_cache.restype = C.c_int
        L.qtts_dev_prefix_cache.argtypes = [C.c_void_p, C.c_int]
        L.qtts_dev_prefix_cache_bytes.restype = C.c_size_t
        L.qtts_dev_prefix_cache_bytes.argtypes = [C.c_void_p]
        L.qtts_dev_get_hidden.restype = C.c_int
        L.qtts_dev_get_hidden.argtypes = [C.c_void_p, C.c_int, _fp]
        for f in (L.qtts_hip_prefix_hits, L.qtts_hip_prefix_misses, L.qtts_hip_prefill_rows):
            f.restype = C.c_longlong
            f.argtypes = []
    if hasattr(L, "qtts_hip_econv_case"):
        L.qtts_hip_econv_plan.restype = C.c_int
        L.qtts_hip_econv_plan.argtypes = [C.POINTER(EConvDesc), C.POINTER(EConvPlan)]
        L.qtts_hip_econv_case.restype = C.c_int
        L.qtts_hip_econv_case.argtypes = [C.POINTER(EConvDesc), C.POINTER(EConvPlan), vp]
        L.qtts_hip_enc_op.restype = C.c_int
        L.qtts_hip_enc_op.argtypes = [C.POINTER(EncOp), vp]
        L.qtts_hip_enc_func.restype = C.c_int
        L.qtts_hip_enc_func.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    if hasattr(L, "qtts_hip_rows_gemm_case"):
        L.qtts_hip_rows_gemm_plan.restype = C.c_int
        L.qtts_hip_rows_gemm_plan.argtypes = [C.POINTER(RowsGemmDesc), C.c_size_t, C.c_size_t, C.c_int,
                                              C.POINTER(RowsGemmPlan)]
        L.qtts_hip_rows_gemm_case.restype = C.c_int
        L.qtts_hip_rows_gemm_case.argtypes = [C.POINTER(RowsGemmDesc), C.c_int, C.POINTER(RowsGemmPlan), vp]
    if hasattr(L, "qtts_hip_batch_matvec_plan"):
        L.qtts_hip_batch_matvec_plan.restype = C.c_int
        L.qtts_hip_batch_matvec_plan.argtypes = [C.POINTER(BGemvDesc), C.POINTER(BGemvPlan)]
    _LIB = L
    return L


_libc = C.CDLL("libc.so.6")
_libc.free.argtypes = [C.c_void_p]


def _take_audio(ptr, n):
    if not ptr or n <= 0:
        return None
    a = np.ctypeslib.as_array(C.cast(ptr, _fp), shape=(n,)).copy()
    _libc.free(ptr)
    return a


def set_verbose(v):
    C.c_int.in_dll(lib(), "qwen_tts_verbose").value = int(v)


class QwenTTS:
    """One model on one HIP device (the reference's qwen_tts_ctx_t)."""

    def __init__(self, model_dir, device=0):
        L = lib()
        self.ctx = L.qwen_tts_load_on(model_dir.encode(), int(device))
        if not self.ctx:
            raise RuntimeError(f"qwen_tts_load({model_dir}) failed")
        self.c = self.ctx.contents
        self.cfg = self.c.config
        self._last_nb = 1

    def close(self):
        if self.ctx:
            lib().qwen_tts_free(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, max_tokens=4096, fixed=0, seed=42, temperature=0.9, top_k=50, top_p=1.0, rep=1.05,
                   st_temperature=0.9, st_top_k=50, st_top_p=1.0):
        c = self.c
        c.temperature, c.top_k, c.top_p, c.repetition_penalty = temperature, top_k, top_p, rep
        c.subtalker_temperature, c.subtalker_top_k, c.subtalker_top_p = st_temperature, st_top_k, st_top_p
        c.max_new_tokens, c.fixed_codec_tokens, c.sample_seed = max_tokens, fixed, seed

    def set_kv_cache(self, dtype):
        """Talker KV cache elements from the next generation on: "fp32" / KV_F32
        (default, codes bit-exact against the reference) or "bf16" / KV_BF16
        (half the cache bytes; qwen_tts_set_kv_cache_dtype)."""
        d = {"fp32": KV_F32, "bf16": KV_BF16}.get(dtype, dtype)
        if not isinstance(d, int) or lib().qwen_tts_set_kv_cache_dtype(self.ctx, d) != 0:
            raise ValueError(f"kv cache dtype {dtype!r} (fp32 or bf16)")

    def kv_cache(self):
        return lib().qwen_tts_kv_cache_dtype(self.ctx)

    def state_bytes(self):
        """device bytes of the generation state (qtts_dev_bytes(dev, 1))"""
        return int(lib().qtts_dev_bytes(C.c_void_p(self.c.hip), 1))

    # per-utterance sampling parameters and seeds (include/qwen_tts.h); one-shot like forcing
    _SAMPLING_KEYS = {"temperature": "temperature", "top_k": "top_k", "top_p": "top_p", "rep": "repetition_penalty",
                      "st_temperature": "subtalker_temperature", "st_top_k": "subtalker_top_k",
                      "st_top_p": "subtalker_top_p", "seed": "sample_seed"}

    def set_utterance_sampling(self, per):
        """per[i]: a dict for utterance i of the next generate* call (slot i of
        a batch, utterance i in input order of generate_queue) with the keys of
        set_params -- temperature, top_k, top_p, rep, st_temperature, st_top_k,
        st_top_p, seed; missing keys take the ctx's current values.
        ValueError when refused (no sets, a non-finite value, top_p <= 0,
        rep <= 0, an unknown key)."""
        arr = (Sampling * max(len(per), 1))()
        for i, d in enumerate(per):
            if lib().qwen_tts_sampling_defaults(self.ctx, C.byref(arr[i])) != 0:
                raise ValueError("set_utterance_sampling: no device model")
            for k, v in d.items():
                if k not in self._SAMPLING_KEYS:
                    raise ValueError(f"set_utterance_sampling: unknown key {k!r}")
                setattr(arr[i], self._SAMPLING_KEYS[k], v)
        if lib().qwen_tts_set_utterance_sampling(self.ctx, len(per), arr) != 0:
            raise ValueError("set_utterance_sampling refused (see stderr)")

    # instruct / voice design (include/qwen_tts.h); one-shot like the sampling sets
    def instruct_prompt(self, instruct):
        """ids of "<|im_start|>user\\n{instruct}<|im_end|>\\n" through the model
        dir's tokenizer (qwen_tts_instruct_prompt); None on error."""
        p = lib().qwen_tts_instruct_prompt(self.ctx, instruct.encode("utf-8"))
        if not p:
            return None
        csv = C.string_at(p).decode()
        _libc.free(C.c_void_p(p))
        return [int(t) for t in csv.split(",")] if csv else []

    def set_utterance_instruct(self, per):
        """per[i]: the instruct ids (a list, or None / [] for none) of utterance
        i of the next generate / generate_stream / generate_batch[_stream] /
        generate_queue[_stream] call; they stand in front of its prompt rows.
        Voice design: the same with speaker None.  ValueError when refused."""
        arr = (C.c_char_p * max(len(per), 1))()
        for i, ids in enumerate(per):
            arr[i] = ",".join(str(int(t)) for t in ids).encode() if ids is not None and len(ids) else None
        if lib().qwen_tts_set_utterance_instruct(self.ctx, len(per), arr) != 0:
            raise ValueError("set_utterance_instruct refused (see stderr)")

    # the device's instruct prefix cache (include/qtts_hip.h)
    def prefix_cache(self, max_entries):
        """capacity in entries; evicts down to it, 0 clears and switches it off"""
        _ok(lib().qtts_dev_prefix_cache(C.c_void_p(self.c.hip), int(max_entries)), "qtts_dev_prefix_cache")

    def prefix_cache_bytes(self):
        return int(lib().qtts_dev_prefix_cache_bytes(C.c_void_p(self.c.hip)))

    @staticmethod
    def prefix_counters():
        """(hits, misses, prefill rows) since the library loaded"""
        L = lib()
        return int(L.qtts_hip_prefix_hits()), int(L.qtts_hip_prefix_misses()), int(L.qtts_hip_prefill_rows())

    # teacher forcing, the free-draw record and logit taps (include/qwen_tts.h).
    # Arming is one-shot: the next generate* call consumes it.
    def force_codes(self, codes, slot=0):
        """Slot `slot` of the next generate* call continues on `codes`
        [frames, groups] (an entry < 0 leaves that draw free, later frames are
        free): every draw runs as always, a forced entry then replaces its
        result.  ValueError when refused (an id out of range)."""
        c = np.ascontiguousarray(codes, np.int32).reshape(-1, self.cfg.num_code_groups)
        if lib().qwen_tts_force_codes(self.ctx, int(slot), c.ctypes.data_as(_ip), c.shape[0]) != 0:
            raise ValueError("force_codes refused (see stderr)")

    def tap_draw(self, frame, group, slot=0):
        """Record the sampler's inputs at draw (frame, group) of `slot` in the
        next generate* call; at most MAX_TAPS per run.  Returns the tap index."""
        i = lib().qwen_tts_tap_draw(self.ctx, int(slot), int(frame), int(group))
        if i < 0:
            raise ValueError("tap_draw refused (see stderr)")
        return i

    def last_drawn(self, slot=0):
        """The free-draw record of the last armed call for `slot`: the id the
        sampler itself produced at every draw, int32 [frames, groups], -1 where
        no draw happened; rows up to the last one with a draw.  None when the
        last call was not armed."""
        cap = max(int(self.c.max_new_tokens), int(self.c.fixed_codec_tokens), 1) + 1
        buf = np.full((cap, self.cfg.num_code_groups), -1, np.int32)
        k = lib().qwen_tts_last_drawn(self.ctx, int(slot), buf.ctypes.data_as(_ip), cap)
        if k < 0:
            return None
        rows = np.nonzero((buf[:k] >= 0).any(axis=1))[0]
        return buf[:rows[-1] + 1 if len(rows) else 0].copy()

    def tap_result(self, i):
        """Tap i of the last armed call: (logits float32 [n], rng_bits, drawn
        id) -- the values the draw saw, the RNG state before it and the id the
        sampler produced -- or None if that draw never happened."""
        n = max(self.cfg.talker_vocab_size, self.cfg.subtalker_vocab_size)
        buf = np.zeros(n, np.float32)
        bits, tok = C.c_uint(0), C.c_int(0)
        k = lib().qwen_tts_tap_result(self.ctx, int(i), buf.ctypes.data_as(_fp), n, C.byref(bits), C.byref(tok))
        if k < 0:
            return None
        return buf[:k].copy(), int(bits.value), int(tok.value)

    def get_kv(self, layer, b, pos0, n):
        """(k, v) fp32 [n, kv_heads * head_dim]: talker cache rows [pos0, pos0 + n)
        of `layer`, slot b (qtts_dev_get_kv; bf16 rows widened exactly)."""
        w = self.cfg.talker_kv_heads * self.cfg.talker_head_dim
        k = np.zeros((n, w), np.float32)
        v = np.zeros((n, w), np.float32)
        rc = lib().qtts_dev_get_kv(C.c_void_p(self.c.hip), int(layer), int(b), int(pos0), int(n),
                                   k.ctypes.data_as(_fp), v.ctypes.data_as(_fp))
        if rc != 0:
            raise ValueError(f"get_kv(layer={layer}, b={b}, pos0={pos0}, n={n}) out of range")
        return k, v

    def get_attn(self, slots, att=True):
        """(qkv [slots, (NH + 2 KV) HD], att [slots, NH HD] or None): the last
        talker layer's decode attention input / output of the most recent
        talker pass (qtts_dev_get_attn); `slots` = the slots of that run."""
        c = self.cfg
        qkv = np.zeros((slots, (c.talker_heads + 2 * c.talker_kv_heads) * c.talker_head_dim), np.float32)
        out = np.zeros((slots, c.talker_heads * c.talker_head_dim), np.float32) if att else None
        rc = lib().qtts_dev_get_attn(C.c_void_p(self.c.hip), qkv.ctypes.data_as(_fp),
                                     out.ctypes.data_as(_fp) if att else None)
        if rc != 0:
            raise RuntimeError("get_attn: no merged attention output from the last talker pass")
        return qkv, out

    def generate(self, ids, speaker=None, language=None):
        csv = ",".join(str(int(i)) for i in ids).encode()
        n = C.c_int(0)
        p = lib().qwen_tts_generate(self.ctx, csv, speaker.encode() if speaker else None,
                                    language.encode() if language else None, C.byref(n))
        return _take_audio(p, n.value)

    def generate_voice_clone(self, ids, ref_ids=None, ref_codes=None, spk_embed=None, language=None,
                             non_streaming=False):
        """Voice clone from reference codes [T, 16] (+ the reference text ids)
        and / or a speaker x-vector (include/qwen_tts.h
        qwen_tts_generate_voice_clone; the Python reference's
        generate_voice_clone minus its audio encoders)."""
        csv = ",".join(str(int(i)) for i in ids).encode()
        rcsv = ",".join(str(int(i)) for i in ref_ids).encode() if ref_ids is not None else None
        rc = None if ref_codes is None else np.ascontiguousarray(ref_codes, np.int32)
        sv = None if spk_embed is None else np.ascontiguousarray(spk_embed, np.float32)
        n = C.c_int(0)
        p = lib().qwen_tts_generate_voice_clone(
            self.ctx, csv, rcsv, None if rc is None else rc.ctypes.data_as(_ip), 0 if rc is None else rc.shape[0],
            None if sv is None else sv.ctypes.data_as(_fp), language.encode() if language else None,
            int(non_streaming), C.byref(n))
        return _take_audio(p, n.value)

    def generate_voice_clone_batch(self, id_lists, ref_id_lists, ref_codes, spk_embeds=None, languages=None,
                                   non_streaming=False):
        """nb voice-clone utterances in lock step (BASELINE C5).  Returns (rc, [audio])."""
        nb = len(id_lists)
        enc = lambda ids: ",".join(str(int(i)) for i in ids).encode() if ids is not None else None
        tx = (C.c_char_p * nb)(*[enc(i) for i in id_lists])
        rt = (C.c_char_p * nb)(*[enc(i) for i in (ref_id_lists or [None] * nb)])
        keep = [None if c is None else np.ascontiguousarray(c, np.int32) for c in (ref_codes or [None] * nb)]
        rc = (_ip * nb)(*[None if c is None else c.ctypes.data_as(_ip) for c in keep])
        nr = (C.c_int * nb)(*[0 if c is None else c.shape[0] for c in keep])
        sk = [None if v is None else np.ascontiguousarray(v, np.float32) for v in (spk_embeds or [None] * nb)]
        sv = (_fp * nb)(*[None if v is None else v.ctypes.data_as(_fp) for v in sk])
        lg = (C.c_char_p * nb)(*[(s.encode() if s else None) for s in (languages or [None] * nb)])
        out = (C.c_void_p * nb)()
        ns = (C.c_int * nb)()
        r = lib().qwen_tts_generate_voice_clone_batch(self.ctx, nb, tx, rt, rc, nr, sv, lg, int(non_streaming), out,
                                                      ns)
        return r, [_take_audio(out[i], ns[i]) for i in range(nb)]

    def generate_voice_clone_batch_stream(self, id_lists, ref_id_lists, ref_codes, spk_embeds=None, languages=None,
                                          non_streaming=False, chunk_frames=4, on_chunk=None):
        """generate_voice_clone_batch with every utterance streamed
        (qwen_tts_generate_voice_clone_batch_stream): on_chunk(b, np.ndarray)
        gets slot b's chunks as they are decoded.  Returns (rc, [audio])."""
        nb = len(id_lists)
        enc = lambda ids: ",".join(str(int(i)) for i in ids).encode() if ids is not None else None
        tx = (C.c_char_p * nb)(*[enc(i) for i in id_lists])
        rt = (C.c_char_p * nb)(*[enc(i) for i in (ref_id_lists or [None] * nb)])
        keep = [None if c is None else np.ascontiguousarray(c, np.int32) for c in (ref_codes or [None] * nb)]
        rc = (_ip * nb)(*[None if c is None else c.ctypes.data_as(_ip) for c in keep])
        nr = (C.c_int * nb)(*[0 if c is None else c.shape[0] for c in keep])
        sk = [None if v is None else np.ascontiguousarray(v, np.float32) for v in (spk_embeds or [None] * nb)]
        sv = (_fp * nb)(*[None if v is None else v.ctypes.data_as(_fp) for v in sk])
        lg = (C.c_char_p * nb)(*[(s.encode() if s else None) for s in (languages or [None] * nb)])
        out = (C.c_void_p * nb)()
        ns = (C.c_int * nb)()

        def _cb(i, p, k, u):
            if on_chunk is not None:
                on_chunk(int(i), np.ctypeslib.as_array(p, shape=(k,)).copy())
        cb = BATCH_AUDIO_CB(_cb)
        r = lib().qwen_tts_generate_voice_clone_batch_stream(self.ctx, nb, tx, rt, rc, nr, sv, lg, int(non_streaming),
                                                             int(chunk_frames), cb, None, out, ns)
        self._last_nb = nb
        return r, [_take_audio(out[i], ns[i]) for i in range(nb)]

    def generate_voice_clone_audio_batch_stream(self, id_lists, ref_wavs, ref_id_lists=None, languages=None,
                                                x_vector_only=None, non_streaming=False, chunk_frames=4,
                                                on_chunk=None):
        """generate_voice_clone_audio_batch with every utterance streamed
        (qwen_tts_generate_voice_clone_audio_batch_stream).  Returns (rc, [audio])."""
        nb = len(id_lists)
        enc = lambda ids: ",".join(str(int(i)) for i in ids).encode() if ids is not None else None
        tx = (C.c_char_p * nb)(*[enc(i) for i in id_lists])
        rt = (C.c_char_p * nb)(*[enc(i) for i in (ref_id_lists or [None] * nb)])
        ws, wp, ns = self._wav_args(ref_wavs)
        lg = (C.c_char_p * nb)(*[(s.encode() if s else None) for s in (languages or [None] * nb)])
        xo = (C.c_int * nb)(*[int(bool(v)) for v in (x_vector_only or [False] * nb)])
        out = (C.c_void_p * nb)()
        on = (C.c_int * nb)()

        def _cb(i, p, k, u):
            if on_chunk is not None:
                on_chunk(int(i), np.ctypeslib.as_array(p, shape=(k,)).copy())
        cb = BATCH_AUDIO_CB(_cb)
        r = lib().qwen_tts_generate_voice_clone_audio_batch_stream(self.ctx, nb, tx, rt, wp, ns, lg, xo,
                                                                   int(non_streaming), int(chunk_frames), cb, None,
                                                                   out, on)
        self._last_nb = nb
        return r, [_take_audio(out[i], on[i]) for i in range(nb)]

    # ---- voice-clone audio encoders (include/qtts_hip.h qtts_dev_speaker_embed / _encode_audio)
    def encoders_available(self):
        """bit 0: speaker encoder, bit 1: 12 Hz encoder."""
        return lib().qtts_dev_enc_available(C.c_void_p(self.c.hip))

    @staticmethod
    def _wav_args(wavs):
        ws = [np.ascontiguousarray(w, np.float32) for w in wavs]
        nb = len(ws)
        return ws, (_fp * nb)(*[w.ctypes.data_as(_fp) for w in ws]), (C.c_int * nb)(*[w.shape[0] for w in ws])

    def speaker_embed(self, wavs, mel=False):
        """x-vectors [nb, talker_hidden] of 24 kHz waveforms (one launch chain
        for the batch, each utterance at its own length); with mel=True also
        the list of [128, T_b] log-mels."""
        ws, wp, ns = self._wav_args(wavs)
        nb = len(ws)
        out = np.zeros((nb, self.cfg.talker_hidden), np.float32)
        T = [(w.shape[0] - 256) // 256 + 1 for w in ws]
        mbuf = np.zeros(sum(128 * t for t in T), np.float32) if mel else None
        rc = lib().qtts_dev_speaker_embed(C.c_void_p(self.c.hip), nb, wp, ns, out.ctypes.data_as(_fp),
                                          mbuf.ctypes.data_as(_fp) if mel else None)
        if rc != 0:
            raise RuntimeError(f"speaker encoder failed (rc={rc})")
        if not mel:
            return out
        mels, o = [], 0
        for t in T:
            mels.append(mbuf[o:o + 128 * t].reshape(128, t).copy())
            o += 128 * t
        return out, mels

    def encode_audio(self, wavs, latent=False):
        """12 Hz codes of 24 kHz waveforms, batch-encoded zero-padded to the
        longest: list of [ceil(n / 1920), 16] int arrays (+ pre-quantizer
        latents [hidden, frames] with latent=True)."""
        ws, wp, ns = self._wav_args(wavs)
        nb = len(ws)
        maxT = max(-(-w.shape[0] // 1920) for w in ws)
        codes = np.zeros((nb, maxT, 16), np.int32)
        frames = (C.c_int * nb)()
        hid = None
        lat = None
        if latent:
            import json
            with open(os.path.join(self.c.model_dir.decode(), "speech_tokenizer", "config.json")) as f:
                hid = json.load(f).get("encoder_config", {}).get("hidden_size", 512)
            lat = np.zeros((nb, hid, maxT), np.float32)
        rc = lib().qtts_dev_encode_audio(C.c_void_p(self.c.hip), nb, wp, ns, codes.ctypes.data_as(_ip), maxT, frames,
                                         lat.ctypes.data_as(_fp) if latent else None)
        if rc != 0:
            raise RuntimeError(f"audio encoder failed (rc={rc})")
        cl = [codes[b, :frames[b]].copy() for b in range(nb)]
        if not latent:
            return cl
        return cl, [lat[b, :, :frames[b]].copy() for b in range(nb)]

    def speaker_embedding_api(self, wav):
        """qwen_tts_speaker_embedding (the public C API)."""
        w = np.ascontiguousarray(wav, np.float32)
        n = C.c_int(0)
        p = lib().qwen_tts_speaker_embedding(self.ctx, w.ctypes.data_as(_fp), w.shape[0], C.byref(n))
        return _take_audio(p, n.value)

    def encode_audio_api(self, wav):
        """qwen_tts_encode_audio (the public C API): [frames, 16] or None."""
        w = np.ascontiguousarray(wav, np.float32)
        n = C.c_int(0)
        p = lib().qwen_tts_encode_audio(self.ctx, w.ctypes.data_as(_fp), w.shape[0], C.byref(n))
        if not p:
            return None
        a = np.ctypeslib.as_array(C.cast(p, _ip), shape=(n.value * 16,)).reshape(n.value, 16).copy()
        _libc.free(C.c_void_p(p))
        return a

    def generate_voice_clone_audio(self, ids, ref_wav, ref_ids=None, language=None, x_vector_only=False,
                                   non_streaming=False):
        """Voice clone from reference audio (qwen_tts_generate_voice_clone_audio)."""
        csv = ",".join(str(int(i)) for i in ids).encode()
        rcsv = ",".join(str(int(i)) for i in ref_ids).encode() if ref_ids is not None else None
        w = np.ascontiguousarray(ref_wav, np.float32)
        n = C.c_int(0)
        p = lib().qwen_tts_generate_voice_clone_audio(self.ctx, csv, rcsv, w.ctypes.data_as(_fp), w.shape[0],
                                                      language.encode() if language else None, int(x_vector_only),
                                                      int(non_streaming), C.byref(n))
        return _take_audio(p, n.value)

    def generate_voice_clone_audio_stream(self, ids, ref_wav, ref_ids=None, language=None, x_vector_only=False,
                                          non_streaming=False, chunk_frames=4, on_chunk=None):
        """Streaming voice clone from reference audio; first packet counts the encode."""
        csv = ",".join(str(int(i)) for i in ids).encode()
        rcsv = ",".join(str(int(i)) for i in ref_ids).encode() if ref_ids is not None else None
        w = np.ascontiguousarray(ref_wav, np.float32)
        n = C.c_int(0)

        def _cb(p, k, u):
            if on_chunk is not None:
                on_chunk(np.ctypeslib.as_array(p, shape=(k,)).copy())
        cb = AUDIO_CB(_cb)
        p = lib().qwen_tts_generate_voice_clone_audio_stream(
            self.ctx, csv, rcsv, w.ctypes.data_as(_fp), w.shape[0], language.encode() if language else None,
            int(x_vector_only), int(non_streaming), int(chunk_frames), cb, None, C.byref(n))
        return _take_audio(p, n.value)

    def generate_voice_clone_audio_batch(self, id_lists, ref_wavs, ref_id_lists=None, languages=None,
                                         x_vector_only=None, non_streaming=False):
        """nb voice clones from reference audio in lock step (BASELINE C5 as
        stated: ref-audio encode + decode + codec).  Returns (rc, [audio])."""
        nb = len(id_lists)
        enc = lambda ids: ",".join(str(int(i)) for i in ids).encode() if ids is not None else None
        tx = (C.c_char_p * nb)(*[enc(i) for i in id_lists])
        rt = (C.c_char_p * nb)(*[enc(i) for i in (ref_id_lists or [None] * nb)])
        ws, wp, ns = self._wav_args(ref_wavs)
        lg = (C.c_char_p * nb)(*[(s.encode() if s else None) for s in (languages or [None] * nb)])
        xo = (C.c_int * nb)(*[int(bool(v)) for v in (x_vector_only or [False] * nb)])
        out = (C.c_void_p * nb)()
        on = (C.c_int * nb)()
        r = lib().qwen_tts_generate_voice_clone_audio_batch(self.ctx, nb, tx, rt, wp, ns, lg, xo, int(non_streaming),
                                                            out, on)
        return r, [_take_audio(out[i], on[i]) for i in range(nb)]

    def generate_batch(self, id_lists, speakers=None, languages=None):
        nb = len(id_lists)
        tx = (C.c_char_p * nb)(*[",".join(str(int(i)) for i in ids).encode() for ids in id_lists])
        sp = (C.c_char_p * nb)(*[(s.encode() if s else None) for s in (speakers or [None] * nb)])
        lg = (C.c_char_p * nb)(*[(s.encode() if s else None) for s in (languages or [None] * nb)])
        out = (C.c_void_p * nb)()
        ns = (C.c_int * nb)()
        rc = lib().qwen_tts_generate_batch(self.ctx, nb, tx, sp, lg, out, ns)
        self._last_nb = nb
        audio = [_take_audio(out[i], ns[i]) for i in range(nb)]
        return rc, audio

    def generate_queue(self, id_lists, speakers=None, languages=None, slots=8, next_fn=None):
        """Work queue (qwen_tts_generate_queue): the utterances on at most
        `slots` lock-step slots, each freed slot refilled with the next
        utterance inside the live batch.  next_fn() (optional) returns the index
        of the next utterance to admit or -1 (e.g. a counter shared by several
        GPUs' processes); default: in order.  Returns (rc, [audio or None])."""
        nq = len(id_lists)
        tx = (C.c_char_p * nq)(*[",".join(str(int(i)) for i in ids).encode() for ids in id_lists])
        sp = (C.c_char_p * nq)(*[(s.encode() if s else None) for s in (speakers or [None] * nq)])
        lg = (C.c_char_p * nq)(*[(s.encode() if s else None) for s in (languages or [None] * nq)])
        out = (C.c_void_p * nq)()
        ns = (C.c_int * nq)()
        cb = QUEUE_NEXT_CB(lambda u: int(next_fn())) if next_fn is not None else QUEUE_NEXT_CB()
        rc = lib().qwen_tts_generate_queue(self.ctx, nq, tx, sp, lg, int(slots), cb, None, out, ns)
        return rc, [_take_audio(out[i], ns[i]) for i in range(nq)]

    def generate_queue_stream(self, id_lists, speakers=None, languages=None, slots=8, next_fn=None, chunk_frames=4,
                              on_chunk=None):
        """generate_queue with every utterance streamed (qwen_tts_generate_queue_stream):
        on_chunk(u, np.ndarray) gets utterance u's chunks (u in input order) as
        they are decoded, whatever slot it runs on.  Returns (rc, [audio or None])."""
        nq = len(id_lists)
        tx = (C.c_char_p * nq)(*[",".join(str(int(i)) for i in ids).encode() for ids in id_lists])
        sp = (C.c_char_p * nq)(*[(s.encode() if s else None) for s in (speakers or [None] * nq)])
        lg = (C.c_char_p * nq)(*[(s.encode() if s else None) for s in (languages or [None] * nq)])
        out = (C.c_void_p * nq)()
        ns = (C.c_int * nq)()
        ncb = QUEUE_NEXT_CB(lambda u: int(next_fn())) if next_fn is not None else QUEUE_NEXT_CB()

        def _cb(i, p, k, u):
            if on_chunk is not None:
                on_chunk(int(i), np.ctypeslib.as_array(p, shape=(k,)).copy())
        cb = BATCH_AUDIO_CB(_cb)
        rc = lib().qwen_tts_generate_queue_stream(self.ctx, nq, tx, sp, lg, int(slots), ncb, None, int(chunk_frames),
                                                  cb, None, out, ns)
        return rc, [_take_audio(out[i], ns[i]) for i in range(nq)]

    def queue_codes(self, i):
        """codes [frames, groups] of utterance i of the last generate_queue (None: not decoded here)"""
        n = lib().qwen_tts_queue_codes(self.ctx, int(i), None, 1 << 30)
        if n < 0:
            return None
        buf = np.zeros((max(n, 1), self.cfg.num_code_groups), np.int32)
        lib().qwen_tts_queue_codes(self.ctx, int(i), buf.ctypes.data_as(_ip), n)
        return buf[:n].copy()

    def queue_stats(self):
        """{slots, frames, refills, used, occupancy, stop_reason[], frames_per_utt[]} of the last generate_queue"""
        c = self.c
        n = c.queue_n
        launched = c.queue_frames_launched
        rl = int(c.queue_rows_launched)
        return {"slots": c.queue_slots, "frames": launched, "refills": c.queue_refills,
                "used": int(c.queue_slot_frames_used), "rows_launched": rl,
                "occupancy": (c.queue_slot_frames_used / rl) if rl else 0.0,
                "occupancy_full_width": (c.queue_slot_frames_used / (c.queue_slots * launched))
                if launched and c.queue_slots else 0.0,
                "stop_reason": [c.queue_stop_reason[i] for i in range(n)] if n else [],
                "frames_per_utt": [c.queue_frames[i] for i in range(n)] if n else [],
                "slot": [c.queue_slot[i] for i in range(n)] if n else []}

    def generate_stream(self, ids, speaker=None, language=None, chunk_frames=4, on_chunk=None):
        """Streaming generation; on_chunk(np.ndarray) gets each audio chunk as
        it is decoded.  Returns the whole utterance."""
        csv = ",".join(str(int(i)) for i in ids).encode()
        n = C.c_int(0)

        def _cb(p, k, u):
            if on_chunk is not None:
                on_chunk(np.ctypeslib.as_array(p, shape=(k,)).copy())
        cb = AUDIO_CB(_cb)
        p = lib().qwen_tts_generate_stream(self.ctx, csv, speaker.encode() if speaker else None,
                                           language.encode() if language else None, int(chunk_frames), cb, None,
                                           C.byref(n))
        return _take_audio(p, n.value)

    def generate_voice_clone_stream(self, ids, ref_ids=None, ref_codes=None, spk_embed=None, language=None,
                                    non_streaming=False, chunk_frames=4, on_chunk=None):
        """Streaming voice clone; chunks start at the reference boundary."""
        csv = ",".join(str(int(i)) for i in ids).encode()
        rcsv = ",".join(str(int(i)) for i in ref_ids).encode() if ref_ids is not None else None
        rc = None if ref_codes is None else np.ascontiguousarray(ref_codes, np.int32)
        sv = None if spk_embed is None else np.ascontiguousarray(spk_embed, np.float32)
        n = C.c_int(0)

        def _cb(p, k, u):
            if on_chunk is not None:
                on_chunk(np.ctypeslib.as_array(p, shape=(k,)).copy())
        cb = AUDIO_CB(_cb)
        p = lib().qwen_tts_generate_voice_clone_stream(
            self.ctx, csv, rcsv, None if rc is None else rc.ctypes.data_as(_ip), 0 if rc is None else rc.shape[0],
            None if sv is None else sv.ctypes.data_as(_fp), language.encode() if language else None,
            int(non_streaming), int(chunk_frames), cb, None, C.byref(n))
        return _take_audio(p, n.value)

    def codec_stream(self, chunks, max_frames=4096):
        """Exact incremental codec decode of a list of [t, 16] code arrays."""
        L = lib()
        if L.qwen_tts_codec_stream_begin(self.ctx, int(max_frames)) != 0:
            raise RuntimeError("codec stream begin failed")
        outs = []
        for c in chunks:
            c = np.ascontiguousarray(c, np.int32)
            o = np.zeros(c.shape[0] * 1920, np.float32)
            k = L.qwen_tts_codec_stream_push(self.ctx, c.ctypes.data_as(_ip), c.shape[0], o.ctypes.data_as(_fp))
            if k != len(o):
                raise RuntimeError(f"codec stream push failed ({k})")
            outs.append(o)
        return outs

    def generate_batch_stream(self, id_lists, speakers=None, languages=None, chunk_frames=4, on_chunk=None):
        """generate_batch with every utterance streamed (qwen_tts_generate_batch_stream):
        on_chunk(i, np.ndarray) gets utterance i's chunks as they are decoded.
        Returns (rc, [audio])."""
        nb = len(id_lists)
        tx = (C.c_char_p * nb)(*[",".join(str(int(i)) for i in ids).encode() for ids in id_lists])
        sp = (C.c_char_p * nb)(*[(s.encode() if s else None) for s in (speakers or [None] * nb)])
        lg = (C.c_char_p * nb)(*[(s.encode() if s else None) for s in (languages or [None] * nb)])
        out = (C.c_void_p * nb)()
        ns = (C.c_int * nb)()

        def _cb(i, p, k, u):
            if on_chunk is not None:
                on_chunk(int(i), np.ctypeslib.as_array(p, shape=(k,)).copy())
        cb = BATCH_AUDIO_CB(_cb)
        rc = lib().qwen_tts_generate_batch_stream(self.ctx, nb, tx, sp, lg, int(chunk_frames), cb, None, out, ns)
        self._last_nb = nb
        return rc, [_take_audio(out[i], ns[i]) for i in range(nb)]

    def _feed_cb(self, feed):
        """the C feed callback around a Python feed(handle, wait); an exception aborts the call"""
        def _cb(fp, wait, u):
            try:
                rc = feed(FeedHandle(fp), int(wait))
                return 0 if rc is None else int(rc)
            except Exception as e:   # (ctypes would print and return 0: the loop must not go on)
                self._feed_error = e
                return -1
        self._feed_error = None
        return TEXT_FEED_CB(_cb)

    def generate_fed_stream(self, feed, speaker=None, language=None, chunk_frames=4, on_chunk=None):
        """Streaming generation that takes its content ids while it runs
        (qwen_tts_generate_fed_stream).  feed(handle, wait) is called before every
        frame launch (wait 0: push what is at hand) and when nothing can advance
        (wait 1: push or close something); handle.push(0, ids), handle.close(0),
        handle.state(0) -> (ids_taken, frames_done, starved).  Return None / 0 to
        go on, < 0 to abort.  Returns the whole utterance, or None."""
        n = C.c_int(0)

        def _cb(p, k, u):
            if on_chunk is not None:
                on_chunk(np.ctypeslib.as_array(p, shape=(k,)).copy())
        cb, fcb = AUDIO_CB(_cb), self._feed_cb(feed)
        p = lib().qwen_tts_generate_fed_stream(self.ctx, speaker.encode() if speaker else None,
                                               language.encode() if language else None, int(chunk_frames), fcb, None,
                                               cb, None, C.byref(n))
        self._last_nb = 1
        if self._feed_error is not None:
            raise self._feed_error
        return _take_audio(p, n.value) if p else None

    def generate_fed_batch_stream(self, nb, feed, speakers=None, languages=None, chunk_frames=4, on_chunk=None):
        """nb fed utterances in lock-step frames (qwen_tts_generate_fed_batch_stream):
        feed(handle, wait) as generate_fed_stream's with utterance indices 0..nb-1,
        on_chunk(i, np.ndarray) per utterance.  Returns (rc, [audio])."""
        n = max(int(nb), 1)
        sp = (C.c_char_p * n)(*[(s.encode() if s else None) for s in (speakers or [None] * n)])
        lg = (C.c_char_p * n)(*[(s.encode() if s else None) for s in (languages or [None] * n)])
        out = (C.c_void_p * n)()
        ns = (C.c_int * n)()

        def _cb(i, p, k, u):
            if on_chunk is not None:
                on_chunk(int(i), np.ctypeslib.as_array(p, shape=(k,)).copy())
        cb = BATCH_AUDIO_CB(_cb)
        fcb = self._feed_cb(feed) if feed is not None else C.cast(None, TEXT_FEED_CB)
        rc = lib().qwen_tts_generate_fed_batch_stream(self.ctx, int(nb), sp, lg, int(chunk_frames), fcb, None, cb, None,
                                                      out, ns)
        self._last_nb = n
        if feed is not None and self._feed_error is not None:
            raise self._feed_error
        return rc, [(_take_audio(out[i], ns[i]) if out[i] else None) for i in range(min(n, int(nb)) if nb > 0 else 0)]

    def text_held_frames(self):
        """frames a live slot of a fed run was held, process-wide (qtts_hip_text_held_frames)"""
        return int(lib().qtts_hip_text_held_frames())

    def codec_mstream_begin(self, n_streams, max_frames=4096):
        """(re)start n_streams independent exact codec streams; 0 or -1"""
        return lib().qwen_tts_codec_mstream_begin(self.ctx, int(n_streams), int(max_frames))

    def codec_mstream_push(self, streams, codes, any_position=False):
        """T more frames of the distinct streams `streams` (all at one position),
        codes [n, T, 16]: [T * 1920 samples] per stream, or None where the
        library refuses the push (-1; nothing decoded)."""
        st = np.ascontiguousarray(streams, np.int32)
        c = np.ascontiguousarray(codes, np.int32)
        n = len(st)
        T = c.shape[1] if c.ndim == 3 else 0
        outs = [np.zeros(max(T, 1) * 1920, np.float32) for _ in range(n)]
        po = (_fp * max(n, 1))(*[o.ctypes.data_as(_fp) for o in outs])
        fn = lib().qwen_tts_codec_mstream_push_any if any_position else lib().qwen_tts_codec_mstream_push
        k = fn(self.ctx, n, st.ctypes.data_as(_ip), c.ctypes.data_as(_ip), T, po)
        if k < 0:
            return None
        if k != T * 1920:
            raise RuntimeError(f"codec mstream push returned {k}")
        return outs

    def codec_mstream_push_any(self, streams, codes):
        """codec_mstream_push for streams at different positions
        (qwen_tts_codec_mstream_push_any): the same arguments and result"""
        return self.codec_mstream_push(streams, codes, any_position=True)

    def codec_mstream_push_ragged(self, streams, code_list, counts=None, ld_frames=None, fill=0.0):
        """Stream streams[i] advances by its own number of frames in one push
        (qwen_tts_codec_mstream_push_ragged): code_list[i] is its [t_i, 16]
        codes.  Returns [t_i * 1920 samples] per stream, or None where the
        library refuses the push (-1; nothing decoded).  counts / ld_frames
        override what the lists imply (the refusal tests); each output buffer
        is ld_frames * 1920 long, filled with `fill` beforehand, and cut to
        counts[i] * 1920 only when counts is not given."""
        st = np.ascontiguousarray(streams, np.int32)
        n = len(st)
        cl = [np.asarray(c, np.int32).reshape(-1, 16) for c in code_list]
        ld = int(ld_frames) if ld_frames is not None else max([len(c) for c in cl] + [1])
        codes = np.zeros((max(n, 1), ld, 16), np.int32)
        for i, c in enumerate(cl):
            codes[i, :min(len(c), ld)] = c[:ld]
        cn = None if counts is None else np.ascontiguousarray(counts, np.int32)
        cnt = np.asarray([len(c) for c in cl], np.int32) if cn is None else cn
        outs = [np.full(ld * 1920, fill, np.float32) for _ in range(n)]
        po = (_fp * max(n, 1))(*[o.ctypes.data_as(_fp) for o in outs])
        cp = cnt.ctypes.data_as(_ip) if counts is None or len(cnt) else None
        k = lib().qwen_tts_codec_mstream_push_ragged(self.ctx, n, st.ctypes.data_as(_ip), codes.ctypes.data_as(_ip),
                                                     cp, ld, po)
        if k < 0:
            return None
        if k != int(cnt.max()) * 1920:
            raise RuntimeError(f"codec mstream ragged push returned {k}")
        return outs if counts is not None else [o[:int(c) * 1920] for o, c in zip(outs, cnt)]

    def codec_mstream_reset(self, stream):
        """one stream back to position 0, the others untouched; 0 or -1"""
        return lib().qwen_tts_codec_mstream_reset(self.ctx, int(stream))

    def codec_mstream_pos(self, stream):
        """frames decoded so far of a stream (-1: no such stream)"""
        return lib().qtts_dev_codec_mstream_pos(self.c.hip, int(stream))

    def codec_mstream_save(self, stream):
        """a snapshot (opaque handle) of one stream's carried state, the stream
        untouched (qwen_tts_codec_mstream_save); None where the library refuses"""
        p = lib().qwen_tts_codec_mstream_save(self.ctx, int(stream))
        return p or None

    def codec_mstream_restore(self, stream, snap):
        """`stream` continues from the snapshot (qwen_tts_codec_mstream_restore); 0 or -1"""
        return lib().qwen_tts_codec_mstream_restore(self.ctx, int(stream), snap)

    @staticmethod
    def codec_snapshot_free(snap):
        lib().qwen_tts_codec_snapshot_free(snap)

    @staticmethod
    def codec_snapshot_pos(snap):
        """frames the snapshot stands at (-1: NULL, freed, or its context is gone)"""
        return lib().qwen_tts_codec_snapshot_pos(snap)

    # ---- voice handles and the voice-clone work queue (include/qwen_tts.h qwen_tts_voice_*)
    def voice_create(self, ref_ids=None, ref_codes=None, spk_embed=None):
        """A voice handle from reference codes [T, 16] (+ the reference text
        ids) and / or a speaker x-vector; None where the library refuses."""
        rcsv = ",".join(str(int(i)) for i in ref_ids).encode() if ref_ids is not None else None
        rc = None if ref_codes is None else np.ascontiguousarray(ref_codes, np.int32)
        sv = None if spk_embed is None else np.ascontiguousarray(spk_embed, np.float32)
        p = lib().qwen_tts_voice_create(self.ctx, rcsv, None if rc is None else rc.ctypes.data_as(_ip),
                                        0 if rc is None else rc.shape[0],
                                        None if sv is None else sv.ctypes.data_as(_fp))
        return p or None

    def voice_create_audio(self, ref_wav, ref_ids=None, x_vector_only=False):
        """A voice handle from 24 kHz reference audio: the two encoders run once."""
        rcsv = ",".join(str(int(i)) for i in ref_ids).encode() if ref_ids is not None else None
        w = np.ascontiguousarray(ref_wav, np.float32)
        p = lib().qwen_tts_voice_create_audio(self.ctx, rcsv, w.ctypes.data_as(_fp), w.shape[0], int(x_vector_only))
        return p or None

    @staticmethod
    def voice_info(voice):
        """{n_ref_frames, primed} of a handle, None for a NULL one"""
        n, pr = C.c_int(0), C.c_int(0)
        if lib().qwen_tts_voice_info(voice, C.byref(n), C.byref(pr)) != 0:
            return None
        return {"n_ref_frames": n.value, "primed": pr.value}

    @staticmethod
    def voice_free(voice):
        lib().qwen_tts_voice_free(voice)

    def generate_voice_queue(self, id_lists, voices, languages=None, non_streaming=False, slots=8, next_fn=None):
        """generate_queue with utterance i spoken in the cloned voice voices[i]
        (handles of voice_create*, repeats allowed; qwen_tts_generate_voice_queue).
        Returns (rc, [audio or None])."""
        nq = len(id_lists)
        tx = (C.c_char_p * nq)(*[",".join(str(int(i)) for i in ids).encode() for ids in id_lists])
        vs = (C.c_void_p * nq)(*voices) if voices is not None else None
        lg = (C.c_char_p * nq)(*[(s.encode() if s else None) for s in (languages or [None] * nq)])
        out = (C.c_void_p * nq)()
        ns = (C.c_int * nq)()
        cb = QUEUE_NEXT_CB(lambda u: int(next_fn())) if next_fn is not None else QUEUE_NEXT_CB()
        rc = lib().qwen_tts_generate_voice_queue(self.ctx, nq, tx, vs, lg, int(non_streaming), int(slots), cb, None,
                                                 out, ns)
        return rc, [_take_audio(out[i], ns[i]) for i in range(nq)]

    def generate_voice_queue_stream(self, id_lists, voices, languages=None, non_streaming=False, slots=8,
                                    next_fn=None, chunk_frames=4, on_chunk=None):
        """generate_voice_queue with every utterance streamed
        (qwen_tts_generate_voice_queue_stream): on_chunk(u, np.ndarray) as
        generate_queue_stream; the audio starts at the reference boundary.
        Returns (rc, [audio or None])."""
        nq = len(id_lists)
        tx = (C.c_char_p * nq)(*[",".join(str(int(i)) for i in ids).encode() for ids in id_lists])
        vs = (C.c_void_p * nq)(*voices) if voices is not None else None
        lg = (C.c_char_p * nq)(*[(s.encode() if s else None) for s in (languages or [None] * nq)])
        out = (C.c_void_p * nq)()
        ns = (C.c_int * nq)()
        ncb = QUEUE_NEXT_CB(lambda u: int(next_fn())) if next_fn is not None else QUEUE_NEXT_CB()

        def _cb(i, p, k, u):
            if on_chunk is not None:
                on_chunk(int(i), np.ctypeslib.as_array(p, shape=(k,)).copy())
        cb = BATCH_AUDIO_CB(_cb)
        rc = lib().qwen_tts_generate_voice_queue_stream(self.ctx, nq, tx, vs, lg, int(non_streaming), int(slots), ncb,
                                                        None, int(chunk_frames), cb, None, out, ns)
        return rc, [_take_audio(out[i], ns[i]) for i in range(nq)]

    def codec_mstream(self, chunk_lists, max_frames=4096):
        """Exact incremental decode of several code sequences at once:
        chunk_lists[s] is stream s's list of [t, 16] code arrays, the same t
        schedule for every stream.  Returns per stream its list of audio chunks."""
        n = len(chunk_lists)
        if self.codec_mstream_begin(n, max_frames) != 0:
            raise RuntimeError("codec mstream begin failed")
        outs = [[] for _ in range(n)]
        for k in range(len(chunk_lists[0])):
            o = self.codec_mstream_push(np.arange(n), np.stack([np.asarray(cl[k], np.int32) for cl in chunk_lists]))
            if o is None:
                raise RuntimeError("codec mstream push failed")
            for s in range(n):
                outs[s].append(o[s])
        return outs

    def last_codes(self):
        G = self.cfg.num_code_groups
        n = self.c.last_frames
        buf = np.zeros((max(n, 1), G), np.int32)
        k = lib().qwen_tts_last_codes(self.ctx, buf.ctypes.data_as(_ip), n)
        return buf[:k].copy()

    def last_codes_slot(self, slot, max_frames=4096):
        """codes of batch slot `slot` of the last generate_batch (frames x groups)"""
        buf = np.zeros((max_frames, self.cfg.num_code_groups), np.int32)
        k = lib().qwen_tts_last_codes_slot(self.ctx, int(slot), buf.ctypes.data_as(_ip), max_frames)
        if k < 0:
            raise ValueError(f"no batch slot {slot}")
        return buf[:k].copy()

    def last_codes_batch(self, nb=None, max_frames=4096):
        return [self.last_codes_slot(b, max_frames) for b in range(nb if nb is not None else self._last_nb)]

    # stage functions (host pointers)
    def prefill(self, embeds):
        e = np.ascontiguousarray(embeds, np.float32)
        lib().qwen_tts_talker_prefill(self.ctx, e.ctypes.data_as(_fp), e.shape[0])
        return self.hidden()

    def hidden(self):
        h = np.zeros(self.cfg.talker_hidden, np.float32)
        lib().qwen_tts_talker_hidden(self.ctx, h.ctypes.data_as(_fp))
        return h

    def step(self, embed):
        e = np.ascontiguousarray(embed, np.float32)
        lg = np.zeros(self.cfg.talker_vocab_size, np.float32)
        lib().qwen_tts_talker_forward(self.ctx, e.ctypes.data_as(_fp), lg.ctypes.data_as(_fp))
        return lg, self.hidden()

    def subtalker(self, hidden, code0):
        out = np.zeros(self.cfg.num_code_groups, np.int32)
        h = np.ascontiguousarray(hidden, np.float32)
        lib().qwen_tts_subtalker_generate(self.ctx, h.ctypes.data_as(_fp), int(code0), out.ctypes.data_as(_ip))
        return out

    def codec_decode(self, codes):
        c = np.ascontiguousarray(codes, np.int32)
        n = C.c_int(0)
        p = lib().qwen_tts_codec_decode(self.ctx, c.ctypes.data_as(_ip), c.shape[0], C.byref(n))
        return _take_audio(p, n.value)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc})")


class Kernels:
    """Kernel-level entry points of qtts_hip.h on torch device tensors."""

    @staticmethod
    def matvec_bf16(out, A_u16, x, rows, cols, batch=1):
        _ok(lib().qtts_hip_matvec_bf16(_ptr(out), _ptr(A_u16), _ptr(x), rows, cols, batch, _stream()), "matvec")

    @staticmethod
    def rmsnorm_matvec_bf16(out, A_u16, x, w, eps, rows, cols, batch=1):
        _ok(lib().qtts_hip_rmsnorm_matvec_bf16(_ptr(out), _ptr(A_u16), _ptr(x), _ptr(w), eps, rows, cols, batch,
                                               _stream()), "rmsnorm_matvec")

    @staticmethod
    def decode_matvec_bf16(out, A_u16, x, w, eps, rows, cols, batch=1):
        _ok(lib().qtts_hip_decode_matvec_bf16(_ptr(out), _ptr(A_u16), _ptr(x), _ptr(w) if w is not None else None,
                                              eps, rows, cols, batch, _stream()), "decode_matvec")

    @staticmethod
    def resident_matvec_bf16(out, A_u16, x, w, eps, rows, cols, epi=0):
        _ok(lib().qtts_hip_resident_matvec_bf16(_ptr(out), _ptr(A_u16), _ptr(x), _ptr(w) if w is not None else None,
                                                eps, rows, cols, epi, _stream()), "resident_matvec")

    @staticmethod
    def sample_top_k(out_i32, logits, vocab, top_k, top_p, temperature, rng_u32, batch=1):
        _ok(lib().qtts_hip_sample_top_k(_ptr(out_i32), _ptr(logits), vocab, top_k, top_p, temperature,
                                        _ptr(rng_u32), batch, _stream()), "sample")

    @staticmethod
    def causal_conv1d(out, x, w, b, ci, co, k, L, dil=1, groups=1):
        _ok(lib().qtts_hip_causal_conv1d(_ptr(out), _ptr(x), _ptr(w), _ptr(b), ci, co, k, L, dil, groups,
                                         _stream()), "conv1d")

    @staticmethod
    def transposed_conv1d(out, x, w, b, ci, co, k, stride, L):
        _ok(lib().qtts_hip_transposed_conv1d(_ptr(out), _ptr(x), _ptr(w), _ptr(b), ci, co, k, stride, L,
                                             _stream()), "tconv1d")

    @staticmethod
    def snake_beta(out, x, alpha, inv_beta, C_, L):
        _ok(lib().qtts_hip_snake_beta(_ptr(out), _ptr(x), _ptr(alpha), _ptr(inv_beta), C_, L, _stream()), "snake")

    @staticmethod
    def expf_glibc(out, x, n):
        _ok(lib().qtts_hip_expf_glibc(_ptr(out), _ptr(x), n, _stream()), "expf")

    @staticmethod
    def attn_decode(out, qkv, kc, vc, qn_w, kn_w, rope_cos, rope_sin, pos_i32, NH, KV, HD, S, rows, eps, kv_dtype=0):
        """The talker's decode attention (qtts_hip_attn_decode): kc / vc
        [rows, S, KV * HD], float32 for kv_dtype 0, bf16 bit patterns (a 2-byte
        torch dtype) for kv_dtype 1; row pos[r] of each is written."""
        _ok(lib().qtts_hip_attn_decode(_ptr(out), _ptr(qkv), _ptr(kc), _ptr(vc), _ptr(qn_w), _ptr(kn_w),
                                       _ptr(rope_cos), _ptr(rope_sin), _ptr(pos_i32), NH, KV, HD, S, rows, eps,
                                       kv_dtype, _stream()), "attn_decode")

    @staticmethod
    def attn_decode_ex(out, qkv, kc, vc, qn_w, kn_w, rope_cos, rope_sin, pos_i32, NH, KV, HD, S, rows, eps,
                       kv_dtype=0, skip_i32=None):
        """attn_decode with per-row skip flags (qtts_hip_attn_decode_ex): a
        flagged row stores no k / v, its output is computed all the same."""
        _ok(lib().qtts_hip_attn_decode_ex(_ptr(out), _ptr(qkv), _ptr(kc), _ptr(vc), _ptr(qn_w), _ptr(kn_w),
                                          _ptr(rope_cos), _ptr(rope_sin), _ptr(pos_i32), NH, KV, HD, S, rows, eps,
                                          kv_dtype, _ptr(skip_i32), _stream()), "attn_decode_ex")

    @staticmethod
    def attn_cached(out, q, ld_q, kc, vc, qn_w, kn_w, rope_cos, rope_sin, row_b_i32, pos_i32, NH, KV, HD, S, slots,
                    rows, eps, win=0, kv_dtype=0, prep=0):
        """The cached attention (qtts_hip_attn_cached): kc / vc [slots, S,
        KV * HD]; prep 1 runs the prefill's q / k norm + RoPE + cache write on
        fused q|k|v rows first (q rewritten in place), prep 0 takes q and the
        caches as they are; win > 0 is the sliding window."""
        _ok(lib().qtts_hip_attn_cached(_ptr(out), _ptr(q), ld_q, _ptr(kc), _ptr(vc), _ptr(qn_w), _ptr(kn_w),
                                       _ptr(rope_cos), _ptr(rope_sin), _ptr(row_b_i32), _ptr(pos_i32), NH, KV, HD, S,
                                       slots, rows, eps, win, kv_dtype, prep, _stream()), "attn_cached")

    @staticmethod
    def attn_o(part, qkv, kc, vc, qn_w, kn_w, rope_cos, rope_sin, pos_i32, Wo_u16, R, NH, KV, HD, S, rows, eps):
        """The sub-talker's attention + O projection by kv head
        (qtts_hip_attn_o): part [KV, rows, R].  False where the kernel does
        not cover the shape (nothing ran)."""
        rc = lib().qtts_hip_attn_o(_ptr(part), _ptr(qkv), _ptr(kc), _ptr(vc), _ptr(qn_w), _ptr(kn_w), _ptr(rope_cos),
                                   _ptr(rope_sin), _ptr(pos_i32), _ptr(Wo_u16), R, NH, KV, HD, S, rows, eps, _stream())
        if rc == 1:
            return False
        _ok(rc, "attn_o")
        return True

    @staticmethod
    def attn_o_pair(part, qkv, kc, vc, qn_w, kn_w, rope_cos, rope_sin, Wo_u16, R, NH, KV, HD, S, eps, skip_i32=None):
        """The pair form of attn_o (qtts_hip_attn_o_pair): qkv [2, (NH + 2 KV) HD]
        at positions 0 and 1 of one slot, kc / vc [S, KV * HD], part [KV, 2, R].
        False where the kernel does not cover the shape (nothing ran)."""
        rc = lib().qtts_hip_attn_o_pair(_ptr(part), _ptr(qkv), _ptr(kc), _ptr(vc), _ptr(qn_w), _ptr(kn_w),
                                        _ptr(rope_cos), _ptr(rope_sin), _ptr(skip_i32), _ptr(Wo_u16), R, NH, KV, HD,
                                        S, eps, _stream())
        if rc == 1:
            return False
        _ok(rc, "attn_o_pair")
        return True

    @staticmethod
    def resident_matvec_rows_bf16(out, A_u16, x, w, eps, rows, cols, epi=0, part=None, x_new=None, nrows=1):
        """k_gemvw (nrows 1) or its pair form (nrows 2) with the sub-talker
        chain's prologue (qtts_hip_resident_matvec_rows_bf16): x [nrows, cols],
        part [n_part, nrows, cols] added in order, the sum stored to x_new.
        False where the kernel does not cover the shape (nothing ran)."""
        rc = lib().qtts_hip_resident_matvec_rows_bf16(_ptr(out), _ptr(A_u16), _ptr(x), _ptr(w), eps, rows, cols, epi,
                                                      _ptr(part), 0 if part is None else int(part.shape[0]),
                                                      _ptr(x_new), nrows, _stream())
        if rc == 1:
            return False
        _ok(rc, "resident_matvec_rows")
        return True

    @staticmethod
    def bgemv_desc(A_u16, batch, y, x=None, table=None, ids_i32=None, ids_bstride=1, ids_rstride=0, ids_off=0,
                   row_sel_i32=None, part_in=None, norm_w=None, eps=1e-6, xcopy=None, xcopy_normed=False,
                   epi=0, bias=None, kz=0, self_reduce=True, part_out=None):
        """The BGemvDesc of one lock-step batch decode GEMV on `batch` rows.
        A_u16 [rows, cols] bf16 bits.  Source: x [batch, cols] fp32 (+ part_in
        [n, batch, cols] added in order), or a bf16-bit / fp32 table [*, cols]
        gathered by ids_i32[ids_off + b * ids_bstride + row_sel_i32[b] *
        ids_rstride].  y [batch, rows] (epi 4: rows / 2).  kz >= 2: split-K,
        self-reducing into y (epi 3) or, self_reduce False, raw partials to
        part_out [kz, batch, rows]."""
        d = BGemvDesc()
        d.rows, d.cols, d.batch = int(A_u16.shape[0]), int(A_u16.shape[1]), int(batch)
        d.A = _ptr(A_u16)
        if table is not None:
            d.src = 1 if table.element_size() == 2 else 2
            d.table, d.ids = _ptr(table), _ptr(ids_i32)
            d.ids_bstride, d.ids_rstride, d.ids_off = ids_bstride, ids_rstride, ids_off
            d.row_sel = _ptr(row_sel_i32)
        else:
            d.src, d.x, d.ldx = 0, _ptr(x), int(x.stride(0))
        if part_in is not None:
            d.part_in, d.n_part_in = _ptr(part_in), int(part_in.shape[0])
        d.norm_w, d.eps = _ptr(norm_w), eps
        d.xcopy, d.xcopy_normed = _ptr(xcopy), int(bool(xcopy_normed))
        d.epi, d.bias = epi, _ptr(bias)
        d.y, d.ldy = _ptr(y), (int(y.stride(0)) if y is not None else 0)
        d.kz, d.self_reduce, d.part_out = kz, int(bool(self_reduce)), _ptr(part_out)
        return d

    @staticmethod
    def batch_matvec_case(A_u16, batch, y, **kw):
        """One lock-step batch decode GEMV (qtts_hip_batch_matvec_case; 2..16
        rows: k_gemvb / k_gemvm, 17..64: k_gemvx) described as bgemv_desc takes
        it.  False where no batch kernel covers the case."""
        d = Kernels.bgemv_desc(A_u16, batch, y, **kw)
        rc = lib().qtts_hip_batch_matvec_case(C.byref(d), _stream())
        if rc == 1:
            return False
        _ok(rc, "batch_matvec_case")
        return True

    @staticmethod
    def batch_matvec_plan(desc):
        """The batch GEMV planner's answer for a BGemvDesc
        (qtts_hip_batch_matvec_plan; host only, no device needed, the pointers
        only need their alignment): a dict with the kernel's name, its template
        integers, grid, block, LDS bytes and k_gemvm's run-time tpw / cch, or
        None where no batch kernel covers the case."""
        p = BGemvPlan()
        rc = lib().qtts_hip_batch_matvec_plan(C.byref(desc), C.byref(p))
        if rc == 1:
            return None
        _ok(rc, "batch_matvec_plan")
        return dict(kernel=BGEMV_KERNELS[p.kernel], tmpl=list(p.tmpl[:p.n_tmpl]), grid=[p.grid_x, p.grid_y],
                    block=p.block, lds=int(p.lds_bytes), tpw=p.tpw, cch=p.cch)

    @staticmethod
    def _rows_gemm_result(rc, p, who):
        if rc == 1:
            return None
        _ok(rc, who)
        return dict(kernel=RG_NAMES[p.kernel], kz=p.kz, grid=[p.grid_x, p.grid_y, p.grid_z], block=p.block)

    @staticmethod
    def rows_gemm_plan(desc, part_elems=0, plane_elems=0, force=-1):
        """The multi-row GEMMs' launch plan for a RowsGemmDesc with a split
        workspace of part_elems floats and plane_elems bf16 of plane scratch
        (qtts_hip_rows_gemm_plan; host only, no device needed).  force -1: the
        prefill's dispatch, 0: qtts_mgemm, 1 / 2: qtts_pgemm at tile width 128 /
        256.  A dict with the kernel's name, kz, grid and block, or None where
        the (forced) launcher does not cover the shape."""
        p = RowsGemmPlan()
        rc = lib().qtts_hip_rows_gemm_plan(C.byref(desc), part_elems, plane_elems, force, C.byref(p))
        return Kernels._rows_gemm_result(rc, p, "rows_gemm_plan")

    @staticmethod
    def rows_gemm_case(desc, force=-1):
        """Runs one multi-row projection (qtts_hip_rows_gemm_case) with the
        descriptor's own scratch: the plan that ran, or None where the (forced)
        launcher does not cover the shape (nothing ran)."""
        p = RowsGemmPlan()
        rc = lib().qtts_hip_rows_gemm_case(C.byref(desc), force, C.byref(p), _stream())
        return Kernels._rows_gemm_result(rc, p, "rows_gemm_case")

    @staticmethod
    def _econv_result(rc, p, who):
        if rc == -1:
            return None
        _ok(rc, who)
        return dict(rows=p.rows, kz=p.kz, grid=[p.grid_x, p.grid_y, p.grid_z], part_elems=int(p.part_elems))

    @staticmethod
    def econv_plan(desc):
        """launch_econv's plan for an EConvDesc (qtts_hip_econv_plan; host only,
        no device needed): a dict with rows (1: the time-major fast path), kz,
        the grid and the split-K workspace floats, or None where the launcher
        refuses the descriptor."""
        p = EConvPlan()
        return Kernels._econv_result(lib().qtts_hip_econv_plan(C.byref(desc), C.byref(p)), p, "econv_plan")

    @staticmethod
    def econv_case(desc):
        """Runs one k_econv launch through launch_econv (qtts_hip_econv_case):
        the plan that ran, or None on a refusal or a device error."""
        p = EConvPlan()
        return Kernels._econv_result(lib().qtts_hip_econv_case(C.byref(desc), C.byref(p), _stream()), p, "econv_case")

    @staticmethod
    def enc_op(op, inp=(), out=(), n=(), s=(), eps=0.0):
        """One launch of a small encoder kernel (qtts_hip_enc_op): op EO_*, inp /
        out torch tensors (None: NULL), n / s the integers of qtts_hip.h's table.
        True when launched, False when refused."""
        d = EncOp()
        d.op = op
        for i, t in enumerate(inp):
            d.inp[i] = t.data_ptr() if t is not None else None
        for i, t in enumerate(out):
            d.out[i] = t.data_ptr() if t is not None else None
        for i, v in enumerate(n):
            d.n[i] = int(v)
        for i, v in enumerate(s):
            d.s[i] = int(v)
        d.eps = eps
        return lib().qtts_hip_enc_op(C.byref(d), _stream()) == 0

    @staticmethod
    def enc_func(out, x, fn):
        """k_econv's own device functions elementwise (qtts_hip_enc_func): fn 0 erff, 1 expm1f."""
        _ok(lib().qtts_hip_enc_func(_ptr(out), _ptr(x), x.numel(), fn, _stream()), "enc_func")

    @staticmethod
    def sample_top_k_rows(out_i32, logits, vocab, top_k, top_p, temperature, rng_u32, batch=1):
        """sample_top_k with one parameter set per row: top_k / top_p /
        temperature are host sequences of `batch` entries (the per-slot
        sampler, qtts_hip_sample_top_k_rows)."""
        k = np.ascontiguousarray(top_k, np.int32)
        p = np.ascontiguousarray(top_p, np.float32)
        t = np.ascontiguousarray(temperature, np.float32)
        assert k.shape == p.shape == t.shape == (batch,)
        _ok(lib().qtts_hip_sample_top_k_rows(_ptr(out_i32), _ptr(logits), vocab, k.ctypes.data_as(_ip),
                                             p.ctypes.data_as(_fp), t.ctypes.data_as(_fp), _ptr(rng_u32), batch,
                                             _stream()), "sample_top_k_rows")

    @staticmethod
    def sample_nucleus(out_i32, logits, vocab, top_k, top_p, temperature, rng_u32, batch=1, path_i32=None):
        """sample_top_k on the kernel with the nucleus short list
        (qtts_hip_sample_nucleus); path_i32 takes, per row, 1 fast top-k, 2
        nucleus short list, 3 full."""
        _ok(lib().qtts_hip_sample_nucleus(_ptr(out_i32), _ptr(logits), vocab, top_k, top_p, temperature,
                                          _ptr(rng_u32), batch, _stream(),
                                          _ptr(path_i32) if path_i32 is not None else None), "sample_nucleus")

    @staticmethod
    def sample_nucleus_rows(out_i32, path_i32, logits, vocab, top_k, top_p, temperature, rng_u32, batch=1, eos=-1,
                            redraw=False):
        """sample_top_k_rows on the per-slot kernel with the nucleus short
        list (qtts_hip_sample_nucleus_rows); path_i32 (may be None) as in
        sample_nucleus; eos >= 0 and redraw: talker mode before a fixed length
        is reached, so a row that draws eos is redrawn without it."""
        k = np.ascontiguousarray(top_k, np.int32)
        p = np.ascontiguousarray(top_p, np.float32)
        t = np.ascontiguousarray(temperature, np.float32)
        assert k.shape == p.shape == t.shape == (batch,)
        _ok(lib().qtts_hip_sample_nucleus_rows(_ptr(out_i32), _ptr(path_i32) if path_i32 is not None else None,
                                               _ptr(logits), vocab, k.ctypes.data_as(_ip), p.ctypes.data_as(_fp),
                                               t.ctypes.data_as(_fp), _ptr(rng_u32), batch, eos, 1 if redraw else 0,
                                               _stream()), "sample_nucleus_rows")

    @staticmethod
    def sample_slot_launches():
        """per-slot sampler launches enqueued or captured since the library loaded (qtts_hip_sample_slot_launches)"""
        return int(lib().qtts_hip_sample_slot_launches())

    @staticmethod
    def gemv_wide_launches():
        """Wide batch GEMV (k_gemvx) launches enqueued or captured since the library loaded."""
        return int(lib().qtts_hip_gemv_wide_launches())

    @staticmethod
    def xgemm_plan(desc, part_elems=0, force_path=-1):
        """The codec dispatcher's plan for one contraction (qtts_hip_xgemm_plan;
        host only, no device needed): (path, splits), or None where force_path
        does not cover the shape."""
        path, splits = C.c_int(-1), C.c_int(0)
        rc = lib().qtts_hip_xgemm_plan(C.byref(desc), part_elems, force_path, C.byref(path), C.byref(splits))
        if rc == 1:
            return None
        _ok(rc, "xgemm_plan")
        return path.value, splits.value

    @staticmethod
    def xgemm_case(desc, part_elems=0, force_path=-1):
        """Runs one contraction of the codec's GEMM family (qtts_hip_xgemm_case)
        with a split workspace of exactly part_elems floats: (path, splits)
        that ran, or None where force_path does not cover the shape (nothing
        ran)."""
        path, splits = C.c_int(-1), C.c_int(0)
        rc = lib().qtts_hip_xgemm_case(C.byref(desc), part_elems, force_path, C.byref(path), C.byref(splits),
                                       _stream())
        if rc == 1:
            return None
        _ok(rc, "xgemm_case")
        return path.value, splits.value

    @staticmethod
    def xgemm_seg_case(desc, nseg, seg_ldb, seg_ldc, part_elems=0, force_path=-1):
        """The same over the conv forms' stream axis (qtts_hip_xgemm_seg_case):
        nseg column segments of desc.N columns in one launch, segment s at
        B + s * seg_ldb -> C + s * seg_ldc (floats)."""
        path, splits = C.c_int(-1), C.c_int(0)
        rc = lib().qtts_hip_xgemm_seg_case(C.byref(desc), int(nseg), int(seg_ldb), int(seg_ldc), part_elems,
                                           force_path, C.byref(path), C.byref(splits), _stream())
        if rc == 1:
            return None
        _ok(rc, "xgemm_seg_case")
        return path.value, splits.value

    @staticmethod
    def xgemm_func(out, x, fn, alpha=None, inv_beta=None):
        """The codec GEMMs' own device functions elementwise (qtts_hip_xgemm_func):
        fn 0 snake with its sin^2 (x [C, L], alpha / inv_beta [C]), 1 expf, 2 tanhf."""
        ch, ln = (x.shape[0], x.shape[1]) if fn == 0 else (1, x.numel())
        _ok(lib().qtts_hip_xgemm_func(_ptr(out), _ptr(x), _ptr(alpha), _ptr(inv_beta), ch, ln, fn, _stream()),
            "xgemm_func")
