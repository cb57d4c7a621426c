/* codec_precision.c - the precision switches (codec convs, codec linears, talker prefill, prefill attention, voice-clone encoders) of the public API
 * (include/qwen_tts.h).  The value lives in the device model behind ctx->hip;
 * the ctx itself holds nothing of it.  Its own file: qwen_tts.c stays the
 * orchestration that runs against any device layer with the generate ABI. */
#include "../../../include/qtts_hip.h"
#include "../../../include/qwen_tts.h"

int qwen_tts_set_codec_precision(qwen_tts_ctx_t *ctx, int precision) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_set_codec_precision((qtts_dev_t *)ctx->hip, precision);
}

int qwen_tts_codec_precision(qwen_tts_ctx_t *ctx) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_codec_precision((const qtts_dev_t *)ctx->hip);
}

int qwen_tts_set_codec_linear_precision(qwen_tts_ctx_t *ctx, int precision) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_set_codec_linear_precision((qtts_dev_t *)ctx->hip, precision);
}

int qwen_tts_codec_linear_precision(qwen_tts_ctx_t *ctx) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_codec_linear_precision((const qtts_dev_t *)ctx->hip);
}

int qwen_tts_set_prefill_precision(qwen_tts_ctx_t *ctx, int precision) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_set_prefill_precision((qtts_dev_t *)ctx->hip, precision);
}

int qwen_tts_prefill_precision(qwen_tts_ctx_t *ctx) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_prefill_precision((const qtts_dev_t *)ctx->hip);
}

int qwen_tts_set_prefill_attention_precision(qwen_tts_ctx_t *ctx, int precision) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_set_prefill_attention_precision((qtts_dev_t *)ctx->hip, precision);
}

int qwen_tts_prefill_attention_precision(qwen_tts_ctx_t *ctx) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_prefill_attention_precision((const qtts_dev_t *)ctx->hip);
}

int qwen_tts_set_encoder_precision(qwen_tts_ctx_t *ctx, int precision) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_set_encoder_precision((qtts_dev_t *)ctx->hip, precision);
}

int qwen_tts_encoder_precision(qwen_tts_ctx_t *ctx) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_encoder_precision((const qtts_dev_t *)ctx->hip);
}
