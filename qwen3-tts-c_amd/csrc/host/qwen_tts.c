/*
 * qwen_tts.c - C host for the MI355X hot path: config + checkpoint loading,
 * prompt layout, the per-frame decode loop and the public qwen_tts.h API.
 *
 * The arithmetic runs on the GPU through include/qtts_hip.h; this file owns
 * what the reference's c/qwen_tts.c owns on the host side:
 *   - config keys and defaults          (c/qwen_tts.c:235-355)
 *   - speaker / language lookup         (c/qwen_tts.c:1120-1145)
 *   - prompt layout (streaming layout)  (c/qwen_tts.c:1147-1243)
 *   - the generation loop, stop rules, progress callback, stderr lines and
 *     perf counters                     (c/qwen_tts.c:1258-1443)
 */
#define _GNU_SOURCE
#include "../../../include/qwen_tts.h"

#include <dirent.h>
#include <fcntl.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include "../../../include/qtts_hip.h"
#include "bpe.h"
#include "qjson.h"

int qwen_tts_verbose = 0;

static void force_disarm(qwen_tts_ctx_t *ctx);   /* (teacher forcing and taps, before run_batch) */

static double now_ms(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1000.0 + (double)ts.tv_nsec / 1e6;
}


/* ------------------------------------------------------------------ config */
static void read_map(const qj_t *root, const char *path, int *n, char ***names, int **ids) {
    const qj_t *m = qj_path(root, path);
    *n = 0;
    *names = NULL;
    *ids = NULL;
    if (!m || m->type != QJ_OBJ || m->n == 0) return;
    *names = (char **)calloc(m->n, sizeof(char *));
    *ids = (int *)calloc(m->n, sizeof(int));
    for (int i = 0; i < m->n; i++) {
        const qj_t *v = m->items[i];
        int id = -1;
        if (v->type == QJ_NUM) id = (int)v->num;
        else if (v->type == QJ_ARR && v->n > 0 && v->items[0]->type == QJ_NUM) id = (int)v->items[0]->num;
        (*names)[*n] = strdup(m->keys[i]);
        (*ids)[*n] = id;
        (*n)++;
    }
}

static int load_config(qwen_tts_ctx_t *ctx) {
    qwen_tts_config_t *c = &ctx->config;
    char path[1100];
    size_t len = 0;
    snprintf(path, sizeof path, "%s/config.json", ctx->model_dir);
    char *txt = qj_read_file(path, &len);
    if (!txt) { fprintf(stderr, "Error: cannot read %s\n", path); return -1; }
    qj_t *js = qj_parse(txt, len);
    free(txt);
    if (!js) { fprintf(stderr, "Error: cannot parse %s\n", path); return -1; }
#define TI(f, k, d) c->f = qj_int(js, "talker_config." k, d)
    TI(talker_vocab_size, "vocab_size", QWEN_TTS_TALKER_VOCAB);
    TI(talker_hidden, "hidden_size", QWEN_TTS_TALKER_HIDDEN);
    TI(talker_intermediate, "intermediate_size", QWEN_TTS_TALKER_INTERMEDIATE);
    TI(talker_layers, "num_hidden_layers", QWEN_TTS_TALKER_LAYERS);
    TI(talker_heads, "num_attention_heads", QWEN_TTS_TALKER_HEADS);
    TI(talker_kv_heads, "num_key_value_heads", QWEN_TTS_TALKER_KV_HEADS);
    TI(talker_head_dim, "head_dim", 0);
    if (c->talker_head_dim <= 0 && c->talker_heads > 0) c->talker_head_dim = c->talker_hidden / c->talker_heads;
    TI(talker_text_hidden, "text_hidden_size", QWEN_TTS_TALKER_TEXT_HIDDEN);
    TI(talker_text_vocab, "text_vocab_size", QWEN_TTS_TALKER_TEXT_VOCAB);
    TI(num_code_groups, "num_code_groups", QWEN_TTS_NUM_CODE_GROUPS);
    c->talker_rms_norm_eps = qj_float(js, "talker_config.rms_norm_eps", 1e-6f);
    c->talker_rope_theta = qj_float(js, "talker_config.rope_theta", 10000.0f);
    c->mrope_section[0] = 16; c->mrope_section[1] = 16; c->mrope_section[2] = 0;
    qj_ints(js, "talker_config.rope_scaling.mrope_section", c->mrope_section, 3);
    TI(subtalker_vocab_size, "code_predictor_config.vocab_size", QWEN_TTS_SUBTALKER_VOCAB);
    TI(subtalker_hidden, "code_predictor_config.hidden_size", QWEN_TTS_SUBTALKER_HIDDEN);
    TI(subtalker_intermediate, "code_predictor_config.intermediate_size", QWEN_TTS_SUBTALKER_INTERMEDIATE);
    TI(subtalker_layers, "code_predictor_config.num_hidden_layers", QWEN_TTS_SUBTALKER_LAYERS);
    TI(subtalker_heads, "code_predictor_config.num_attention_heads", QWEN_TTS_SUBTALKER_HEADS);
    TI(subtalker_kv_heads, "code_predictor_config.num_key_value_heads", QWEN_TTS_SUBTALKER_KV_HEADS);
    TI(subtalker_head_dim, "code_predictor_config.head_dim", QWEN_TTS_SUBTALKER_HEAD_DIM);
    TI(codec_pad_id, "codec_pad_id", QWEN_TTS_CODEC_PAD);
    TI(codec_bos_id, "codec_bos_id", QWEN_TTS_CODEC_BOS);
    TI(codec_eos_id, "codec_eos_token_id", QWEN_TTS_CODEC_EOS);
    TI(codec_nothink_id, "codec_nothink_id", QWEN_TTS_CODEC_NOTHINK);
    TI(codec_think_id, "codec_think_id", QWEN_TTS_CODEC_THINK);
    TI(codec_think_bos_id, "codec_think_bos_id", QWEN_TTS_CODEC_THINK_BOS);
    TI(codec_think_eos_id, "codec_think_eos_id", QWEN_TTS_CODEC_THINK_EOS);
#undef TI
    read_map(js, "talker_config.spk_id", &c->n_speakers, &c->speaker_names, &c->speaker_ids);
    read_map(js, "talker_config.codec_language_id", &c->n_languages, &c->language_names, &c->language_ids);
    qj_free(js);
    if (c->talker_heads <= 0 || c->talker_kv_heads <= 0 || c->talker_head_dim <= 0) {
        fprintf(stderr, "Error: invalid talker attention config (heads=%d kv_heads=%d head_dim=%d)\n",
                c->talker_heads, c->talker_kv_heads, c->talker_head_dim);
        return -1;
    }
    if (c->talker_heads % c->talker_kv_heads != 0) {
        fprintf(stderr, "Error: talker heads (%d) must be divisible by kv heads (%d)\n", c->talker_heads,
                c->talker_kv_heads);
        return -1;
    }
    if (c->talker_head_dim > 512 || c->subtalker_head_dim > 512) {
        fprintf(stderr, "Error: unsupported head_dim (talker=%d subtalker=%d, max=512)\n", c->talker_head_dim,
                c->subtalker_head_dim);
        return -1;
    }
    if (c->num_code_groups > QWEN_TTS_NUM_CODE_GROUPS) {
        fprintf(stderr, "Error: num_code_groups %d > %d\n", c->num_code_groups, QWEN_TTS_NUM_CODE_GROUPS);
        return -1;
    }

    snprintf(path, sizeof path, "%s/speech_tokenizer/config.json", ctx->model_dir);
    txt = qj_read_file(path, &len);
    if (!txt) { fprintf(stderr, "Error: cannot read %s\n", path); return -1; }
    js = qj_parse(txt, len);
    free(txt);
    if (!js) { fprintf(stderr, "Error: cannot parse %s\n", path); return -1; }
#define DI(f, k, d) c->f = qj_int(js, "decoder_config." k, d)
    DI(codec_num_quantizers, "num_quantizers", QWEN_TTS_CODEC_NUM_QUANTIZERS);
    DI(codec_codebook_size, "codebook_size", QWEN_TTS_CODEC_CODEBOOK_SIZE);
    DI(codec_codebook_dim, "codebook_dim", 128);
    DI(codec_hidden, "hidden_size", QWEN_TTS_CODEC_HIDDEN);
    DI(codec_latent, "latent_dim", QWEN_TTS_CODEC_LATENT);
    DI(codec_layers, "num_hidden_layers", QWEN_TTS_CODEC_LAYERS);
    DI(codec_heads, "num_attention_heads", QWEN_TTS_CODEC_HEADS);
    DI(codec_kv_heads, "num_key_value_heads", QWEN_TTS_CODEC_KV_HEADS);
    DI(codec_intermediate, "intermediate_size", QWEN_TTS_CODEC_INTERMEDIATE);
    DI(codec_sliding_window, "sliding_window", QWEN_TTS_CODEC_SLIDING_WINDOW);
    DI(codec_decoder_dim, "decoder_dim", QWEN_TTS_CODEC_DECODER_DIM);
#undef DI
    c->codec_rms_norm_eps = qj_float(js, "decoder_config.rms_norm_eps", 1e-5f);
    c->codec_layer_scale = qj_float(js, "decoder_config.layer_scale_initial_scale", 0.01f);
    int rates[4] = {8, 5, 4, 3}, ratios[2] = {2, 2};
    qj_ints(js, "decoder_config.upsample_rates", rates, 4);
    qj_ints(js, "decoder_config.upsampling_ratios", ratios, 2);
    memcpy(c->codec_upsample_rates, rates, sizeof rates);
    memcpy(c->codec_upsampling_ratios, ratios, sizeof ratios);
    qj_free(js);
    if (qwen_tts_verbose >= 1) {
        fprintf(stderr, "Config loaded:\n");
        fprintf(stderr, "  Talker: %d layers, hidden=%d, heads=%d/%d, head_dim=%d\n", c->talker_layers,
                c->talker_hidden, c->talker_heads, c->talker_kv_heads, c->talker_head_dim);
        fprintf(stderr, "  Sub-talker: %d layers, hidden=%d, heads=%d/%d, head_dim=%d\n", c->subtalker_layers,
                c->subtalker_hidden, c->subtalker_heads, c->subtalker_kv_heads, c->subtalker_head_dim);
        fprintf(stderr, "  Codec: %d layers, hidden=%d, codebook_dim=%d, decoder_dim=%d\n", c->codec_layers,
                c->codec_hidden, c->codec_codebook_dim, c->codec_decoder_dim);
        fprintf(stderr, "  Speakers: %d, Languages: %d\n", c->n_speakers, c->n_languages);
    }
    return 0;
}

/* ------------------------------------------------------------- checkpoint */
static int cmp_name(const void *a, const void *b) { return strcmp(*(char *const *)a, *(char *const *)b); }

static int is_talker_attn_proj(const char *n) {
    if (strncmp(n, "talker.model.layers.", 20) != 0) return 0;
    const char *s = strstr(n, ".self_attn.");
    return s && s[11] && strchr("qkvo", s[11]) && !strcmp(s + 12, "_proj.weight");
}

/* mmap one .safetensors file and hand every tensor to the device */
static int upload_file(qtts_dev_t *dev, const char *path) {
    int fd = open(path, O_RDONLY);
    if (fd < 0) { fprintf(stderr, "Error: cannot open %s\n", path); return -1; }
    struct stat st;
    if (fstat(fd, &st) < 0 || st.st_size < 8) { close(fd); return -1; }
    size_t size = (size_t)st.st_size;
    uint8_t *base = (uint8_t *)mmap(NULL, size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (base == MAP_FAILED) { fprintf(stderr, "Error: mmap failed for %s\n", path); return -1; }
    uint64_t hlen;
    memcpy(&hlen, base, 8);
    int rc = -1;
    qj_t *hdr = NULL;
    if (hlen + 8 > size || !(hdr = qj_parse((const char *)base + 8, (size_t)hlen)) || hdr->type != QJ_OBJ) {
        fprintf(stderr, "Error: bad safetensors header in %s\n", path);
        goto done;
    }
    const uint8_t *data = base + 8 + hlen;
    for (int i = 0; i < hdr->n; i++) {
        const char *name = hdr->keys[i];
        const qj_t *e = hdr->items[i];
        if (!strcmp(name, "__metadata__")) continue;
        const qj_t *dt = qj_get(e, "dtype"), *sh = qj_get(e, "shape"), *off = qj_get(e, "data_offsets");
        if (!dt || dt->type != QJ_STR || !sh || sh->type != QJ_ARR || !off || off->type != QJ_ARR || off->n != 2) {
            fprintf(stderr, "Error: malformed entry %s in %s\n", name, path);
            goto done;
        }
        int dtype = !strcmp(dt->str, "F32") ? 0 : !strcmp(dt->str, "BF16") ? 1 : !strcmp(dt->str, "F16") ? 2 : -1;
        if (is_talker_attn_proj(name) && dtype != 1) {  /* c/qwen_tts.c:389-393 */
            fprintf(stderr, "Error: tensor %s dtype mismatch: expected BF16, got %s\n", name, dt->str);
            goto done;
        }
        if (dtype < 0) continue;
        int64_t shape[8];
        int nd = sh->n < 8 ? sh->n : 8;
        size_t n = 1;
        for (int k = 0; k < nd; k++) { shape[k] = (int64_t)sh->items[k]->num; n *= (size_t)shape[k]; }
        size_t a = (size_t)off->items[0]->num, b = (size_t)off->items[1]->num;
        size_t esz = dtype == 0 ? 4 : 2;
        if (b < a || b - a != n * esz || 8 + hlen + b > size) {
            fprintf(stderr, "Error: tensor %s has inconsistent size in %s\n", name, path);
            goto done;
        }
        if (qtts_dev_put_tensor(dev, name, data + a, dtype, shape, nd) != 0) goto done;
    }
    rc = 0;
done:
    qj_free(hdr);
    munmap(base, size);
    return rc;
}

static int upload_dir(qtts_dev_t *dev, const char *dir) {
    DIR *d = opendir(dir);
    if (!d) { fprintf(stderr, "Error: cannot open directory %s\n", dir); return -1; }
    char **names = NULL;
    int n = 0, cap = 0;
    struct dirent *ent;
    while ((ent = readdir(d))) {
        const char *dot = strrchr(ent->d_name, '.');
        if (!dot || strcmp(dot, ".safetensors")) continue;
        if (n == cap) { cap = cap ? cap * 2 : 8; names = (char **)realloc(names, cap * sizeof(char *)); }
        names[n++] = strdup(ent->d_name);
    }
    closedir(d);
    if (n == 0) { fprintf(stderr, "Error: no .safetensors files in %s\n", dir); free(names); return -1; }
    qsort(names, n, sizeof(char *), cmp_name);
    int rc = 0;
    for (int i = 0; i < n; i++) {
        char p[1400];
        snprintf(p, sizeof p, "%s/%s", dir, names[i]);
        if (!rc && upload_file(dev, p)) rc = -1;
        free(names[i]);
    }
    free(names);
    return rc;
}

/* Voice-clone encoder config: config.json
 * `speaker_encoder_config` (defaults of Qwen3TTSSpeakerEncoderConfig,
 * configuration_qwen3_tts.py:47-57: enc_dim 1024; it must equal the talker
 * hidden the x-vector takes the place of, else the speaker encoder stays off) and speech_tokenizer/config.json `encoder_config`
 * (transformers MimiConfig defaults).  Returns 1 when either section exists. */
static int load_enc_config(const qwen_tts_ctx_t *ctx, qtts_enc_dims_t *e) {
    memset(e, 0, sizeof *e);
    char path[1100];
    size_t len = 0;
    int have = 0;
    snprintf(path, sizeof path, "%s/config.json", ctx->model_dir);
    char *txt = qj_read_file(path, &len);
    qj_t *js = txt ? qj_parse(txt, len) : NULL;
    free(txt);
    if (js && qj_path(js, "speaker_encoder_config")) have = 1;
#define SI(f, k, d) e->f = qj_int(js, "speaker_encoder_config." k, d)
    SI(mel_dim, "mel_dim", 128);
    SI(enc_dim, "enc_dim", 1024);   /* Qwen3TTSSpeakerEncoderConfig default */
    SI(att_ch, "enc_attention_channels", 128);
    SI(res2net_scale, "enc_res2net_scale", 8);
    SI(se_ch, "enc_se_channels", 128);
#undef SI
    static const int dch[5] = {512, 512, 512, 512, 1536}, dks[5] = {5, 3, 3, 3, 1}, ddl[5] = {1, 2, 3, 4, 1};
    memcpy(e->ch, dch, sizeof dch); memcpy(e->ks, dks, sizeof dks); memcpy(e->dil, ddl, sizeof ddl);
    e->n_ch = 5;
    if (js) {
        int n = qj_ints(js, "speaker_encoder_config.enc_channels", e->ch, 8);
        if (n > 0) e->n_ch = n;
        qj_ints(js, "speaker_encoder_config.enc_kernel_sizes", e->ks, 8);
        qj_ints(js, "speaker_encoder_config.enc_dilations", e->dil, 8);
    }
    qj_free(js);
    snprintf(path, sizeof path, "%s/speech_tokenizer/config.json", ctx->model_dir);
    txt = qj_read_file(path, &len);
    js = txt ? qj_parse(txt, len) : NULL;
    free(txt);
    if (js && qj_path(js, "encoder_config")) have = 1;
#define MI(f, k, d) e->f = qj_int(js, "encoder_config." k, d)
    MI(hidden, "hidden_size", 512);
    MI(n_filters, "num_filters", 64);
    MI(kernel, "kernel_size", 7);
    MI(last_kernel, "last_kernel_size", 3);
    MI(res_kernel, "residual_kernel_size", 3);
    MI(dil_growth, "dilation_growth_rate", 2);
    MI(n_res, "num_residual_layers", 1);
    MI(compress, "compress", 2);
    MI(layers, "num_hidden_layers", 8);
    MI(heads, "num_attention_heads", 8);
    MI(kv_heads, "num_key_value_heads", 8);
    MI(head_dim, "head_dim", 64);
    MI(inter, "intermediate_size", 2048);
    MI(window, "sliding_window", 250);
    MI(n_q, "num_quantizers", 32);
    MI(n_sem, "num_semantic_quantizers", 1);
    MI(cb_size, "codebook_size", 2048);
    MI(vq_dim, "vector_quantization_hidden_dimension", 256);
#undef MI
    e->n_valid = qj_int(js, "encoder_valid_num_quantizers", 16);
    e->norm_eps = qj_float(js, "encoder_config.norm_eps", 1e-5f);
    e->rope_theta = qj_float(js, "encoder_config.rope_theta", 0.f);
    if (e->rope_theta <= 0.f) e->rope_theta = qj_float(js, "encoder_config.rope_parameters.rope_theta", 10000.0f);
    int ratios[4] = {8, 6, 5, 4};
    if (js) qj_ints(js, "encoder_config.upsampling_ratios", ratios, 4);
    memcpy(e->ratios, ratios, sizeof ratios);
    qj_free(js);
    return have;
}

static void dims_of(const qwen_tts_config_t *c, qtts_dims_t *d) {
    memset(d, 0, sizeof *d);
    d->H = c->talker_hidden; d->I = c->talker_intermediate; d->L = c->talker_layers; d->NH = c->talker_heads;
    d->KV = c->talker_kv_heads; d->HD = c->talker_head_dim; d->TH = c->talker_text_hidden;
    d->TV = c->talker_text_vocab; d->V = c->talker_vocab_size; d->G = c->num_code_groups;
    d->Hs = c->subtalker_hidden; d->Is = c->subtalker_intermediate; d->Ls = c->subtalker_layers;
    d->NHs = c->subtalker_heads; d->KVs = c->subtalker_kv_heads; d->HDs = c->subtalker_head_dim;
    d->Vs = c->subtalker_vocab_size;
    d->eps = c->talker_rms_norm_eps; d->theta = c->talker_rope_theta;
    d->cq = c->codec_num_quantizers; d->ccb = c->codec_codebook_size; d->ccbdim = c->codec_codebook_dim;
    d->chid = c->codec_hidden; d->clat = c->codec_latent; d->clayers = c->codec_layers; d->cheads = c->codec_heads;
    d->ckv = c->codec_kv_heads; d->cinter = c->codec_intermediate; d->cwin = c->codec_sliding_window;
    d->cdec = c->codec_decoder_dim;
    memcpy(d->rates, c->codec_upsample_rates, sizeof d->rates);
    memcpy(d->ratios, c->codec_upsampling_ratios, sizeof d->ratios);
    d->ceps = c->codec_rms_norm_eps;
    d->pad_id = c->codec_pad_id; d->bos_id = c->codec_bos_id; d->eos_id = c->codec_eos_id;
}

qwen_tts_ctx_t *qwen_tts_load(const char *model_dir) { return qwen_tts_load_on(model_dir, -1); }

qwen_tts_ctx_t *qwen_tts_load_on(const char *model_dir, int device) {
    double t0 = now_ms();
    qwen_tts_ctx_t *ctx = (qwen_tts_ctx_t *)calloc(1, sizeof(qwen_tts_ctx_t));
    if (!ctx) return NULL;
    snprintf(ctx->model_dir, sizeof ctx->model_dir, "%s", model_dir);
    ctx->temperature = 0.9f;      /* c/qwen_tts.c:871-880 */
    ctx->subtalker_temperature = 0.9f;
    ctx->top_k = 50;
    ctx->subtalker_top_k = 50;
    ctx->top_p = 1.0f;
    ctx->subtalker_top_p = 1.0f;
    ctx->repetition_penalty = 1.05f;
    ctx->max_new_tokens = 4096;
    ctx->fixed_codec_tokens = 0;
    ctx->sample_seed = 42;
    if (load_config(ctx) != 0) { qwen_tts_free(ctx); return NULL; }
    int dev_id = device;
    if (dev_id < 0) {
        const char *e = getenv("QWEN_TTS_HIP_DEVICE");
        dev_id = e ? atoi(e) : 0;
    }
    if (qtts_hip_device_count() <= dev_id) {
        fprintf(stderr, "Error: no HIP device %d available (MI355X / gfx950 required)\n", dev_id);
        qwen_tts_free(ctx);
        return NULL;
    }
    ctx->hip_device = dev_id;
    qtts_dims_t dims;
    dims_of(&ctx->config, &dims);
    qtts_dev_t *dev = qtts_dev_create(&dims, dev_id);
    if (!dev) { qwen_tts_free(ctx); return NULL; }
    ctx->hip = dev;
    qtts_enc_dims_t ed;
    if (load_enc_config(ctx, &ed) && qtts_dev_enc_config(dev, &ed) != 0)   /* not fatal: encoders stay off */
        fprintf(stderr, "Warning: unsupported voice-clone encoder config: encoders disabled\n");
    char cdir[1100];
    snprintf(cdir, sizeof cdir, "%s/speech_tokenizer", model_dir);
    if (upload_dir(dev, model_dir) != 0 || upload_dir(dev, cdir) != 0 || qtts_dev_finalize(dev) != 0) {
        qwen_tts_free(ctx);
        return NULL;
    }
    ctx->tk_x = (float *)calloc(ctx->config.talker_hidden, sizeof(float));
    if (qwen_tts_verbose >= 1)
        fprintf(stderr, "Model loaded in %.1f ms (%.2f GB weights on HIP device %d)\n", now_ms() - t0,
                (double)qtts_dev_bytes(dev, 0) / 1e9, dev_id);
    return ctx;
}

int qwen_tts_set_kv_cache_dtype(qwen_tts_ctx_t *ctx, int dtype) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_set_kv_dtype((qtts_dev_t *)ctx->hip, dtype);
}

int qwen_tts_kv_cache_dtype(qwen_tts_ctx_t *ctx) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_kv_dtype((qtts_dev_t *)ctx->hip);
}

/* the per-utterance results of the last qwen_tts_generate_queue */
static void queue_clear(qwen_tts_ctx_t *ctx) {
    if (ctx->queue_codes)
        for (int i = 0; i < ctx->queue_n; i++) free(ctx->queue_codes[i]);
    free(ctx->queue_codes);
    free(ctx->queue_frames);
    free(ctx->queue_stop_reason);
    free(ctx->queue_slot);
    ctx->queue_codes = NULL;
    ctx->queue_frames = ctx->queue_stop_reason = ctx->queue_slot = NULL;
    ctx->queue_n = 0;
    ctx->queue_frames_launched = 0;
    ctx->queue_slot_frames_used = 0;
    ctx->queue_rows_launched = 0;
    ctx->queue_refills = 0;
    ctx->queue_slots = 0;
}

void qwen_tts_free(qwen_tts_ctx_t *ctx) {
    if (!ctx) return;
    if (ctx->hip) qtts_dev_destroy((qtts_dev_t *)ctx->hip);
    for (int i = 0; i < ctx->config.n_speakers; i++) free(ctx->config.speaker_names[i]);
    free(ctx->config.speaker_names);
    free(ctx->config.speaker_ids);
    for (int i = 0; i < ctx->config.n_languages; i++) free(ctx->config.language_names[i]);
    free(ctx->config.language_names);
    free(ctx->config.language_ids);
    force_disarm(ctx);
    free(ctx->last_codes);
    free(ctx->tk_x);
    queue_clear(ctx);
    qtok_free((qtok_t *)ctx->tokenizer);
    free(ctx);
}

/* ------------------------------------------------------------------ text input (bpe.c) */
int *qwen_tts_tokenize(const char *model_dir, const char *text, int *n_ids) {
    if (n_ids) *n_ids = 0;
    if (!model_dir || !text || !n_ids) return NULL;
    qtok_t *t = qtok_load(model_dir);
    if (!t) return NULL;
    int *ids = NULL;
    const int n = qtok_encode(t, text, &ids);
    qtok_free(t);
    if (n < 0) return NULL;
    *n_ids = n;
    return ids;
}

/* the ids CSV of pre ++ text ++ post through the ctx's tokenizer (malloc'd) */
static char *chat_prompt(qwen_tts_ctx_t *ctx, const char *pre, const char *text, const char *post, const char *what) {
    if (!ctx || !text) return NULL;
    if (!ctx->tokenizer && !(ctx->tokenizer = qtok_load(ctx->model_dir))) return NULL;
    const size_t lp = strlen(pre), lt = strlen(text), lq = strlen(post);
    char *chat = (char *)malloc(lp + lt + lq + 1);
    if (!chat) return NULL;
    memcpy(chat, pre, lp);
    memcpy(chat + lp, text, lt);
    memcpy(chat + lp + lt, post, lq + 1);
    int *ids = NULL;
    const int n = qtok_encode((qtok_t *)ctx->tokenizer, chat, &ids);
    free(chat);
    if (n < 0) return NULL;
    char *csv = (char *)malloc((size_t)n * 12 + 1);
    if (!csv) { free(ids); return NULL; }
    size_t k = 0;
    for (int i = 0; i < n; i++) k += (size_t)sprintf(csv + k, i ? ",%d" : "%d", ids[i]);
    csv[k] = 0;
    free(ids);
    if (qwen_tts_verbose >= 1) fprintf(stderr, "%s: %d tokens (chat template)\n", what, n);
    return csv;
}

char *qwen_tts_text_prompt(qwen_tts_ctx_t *ctx, const char *text) {
    return chat_prompt(ctx, "<|im_start|>assistant\n", text, "<|im_end|>\n<|im_start|>assistant\n", "Text");
}

/* the instruct's chat template (qwen3_tts_model.py:275-276) */
char *qwen_tts_instruct_prompt(qwen_tts_ctx_t *ctx, const char *instruct) {
    return chat_prompt(ctx, "<|im_start|>user\n", instruct, "<|im_end|>\n", "Instruct");
}

void qwen_tts_set_progress_callback(qwen_tts_ctx_t *ctx, qwen_tts_progress_cb cb, void *userdata) {
    ctx->progress_cb = cb;
    ctx->progress_cb_userdata = userdata;
}

/* ------------------------------------------------------------------ prompt */
static int parse_ids(const char *text, int **out) {
    *out = NULL;
    if (!text) return 0;
    int cap = 1;
    for (const char *p = text; *p; p++) cap += *p == ',';
    int *ids = (int *)malloc(cap * sizeof(int)), n = 0;
    const char *p = text;
    while (*p && n < cap) {
        while (*p == ' ' || *p == ',') p++;
        if (!*p) break;
        char *end = NULL;
        long v = strtol(p, &end, 10);
        if (end == p) {
            fprintf(stderr, "Error: invalid token ID near '%s'\n", p);
            free(ids);
            return -1;
        }
        ids[n++] = (int)v;
        p = end;
    }
    *out = ids;
    return n;
}

typedef struct {
    int *text;  /* text ids to project */
    int n_text;
    int *plan;  /* 5 ints per row */
    int nplan;
    int p_len, n_trailing, pad_row;
} prompt_t;

/* Streaming prompt layout of c/qwen_tts.c:1147-1243:
 *   prefill = proj(ids[0:3]),
 *             (tts_pad x (np-2), tts_bos) + codec_emb(prefix[0:np-1]),
 *             proj(ids[3]) + codec_emb(bos)
 *   trailing = proj(ids[4:-5]) ++ tts_eos; tts_pad once exhausted
 * With an instruct (ins, ni > 0) its ni projected rows come first. */
static int build_prompt(const qwen_tts_ctx_t *ctx, const int *ids, int n, int spk, int lang, const int *ins, int ni,
                        int b, prompt_t *pr) {
    const qwen_tts_config_t *c = &ctx->config;
    int prefix[8], np = 0;
    if (lang < 0) {
        prefix[np++] = c->codec_nothink_id; prefix[np++] = c->codec_think_bos_id; prefix[np++] = c->codec_think_eos_id;
    } else {
        prefix[np++] = c->codec_think_id; prefix[np++] = c->codec_think_bos_id; prefix[np++] = lang;
        prefix[np++] = c->codec_think_eos_id;
    }
    if (spk >= 0) prefix[np++] = spk;
    prefix[np++] = c->codec_pad_id;
    prefix[np++] = c->codec_bos_id;
    int nt = (n - 4 - 5) + 1;
    if (nt < 1) nt = 1;
    const int n_own = 7 + (nt - 1);   /* the instruct ids go behind the utterance's own text rows */
    pr->n_text = n_own + ni;
    pr->text = (int *)malloc(pr->n_text * sizeof(int));
    pr->plan = (int *)malloc((size_t)(ni + 3 + np + nt) * 5 * sizeof(int));
    if (!pr->text || !pr->plan) return -1;
    int *t = pr->text;
    t[0] = ids[0]; t[1] = ids[1]; t[2] = ids[2];
    t[3] = QWEN_TTS_TOKEN_TTS_PAD; t[4] = QWEN_TTS_TOKEN_TTS_BOS; t[5] = QWEN_TTS_TOKEN_TTS_EOS; t[6] = ids[3];
    for (int i = 0; i < nt - 1; i++) t[7 + i] = ids[4 + i];
    for (int i = 0; i < ni; i++) t[n_own + i] = ins[i];
    int k = 0;
#define ROW(src, cid, kind, slot) do { int *r_ = pr->plan + 5 * k++; r_[0] = src; r_[1] = cid; r_[2] = kind; r_[3] = b; r_[4] = slot; } while (0)
    /* the instruct rows (M.py:2075-2080, 2236-2237): proj(instruct ids) alone, in
     * front of everything; kind 2 = a prefill row of the cacheable prefix */
    for (int i = 0; i < ni; i++) ROW(n_own + i, -1, 2, i);
    for (int i = 0; i < 3; i++) ROW(i, -1, 0, ni + i);
    for (int i = 0; i < np - 1; i++) ROW(i < np - 2 ? 3 : 4, prefix[i], 0, ni + 3 + i);
    ROW(6, c->codec_bos_id, 0, ni + 3 + np - 1);
    for (int i = 0; i < nt - 1; i++) ROW(7 + i, -1, 1, i);
    ROW(5, -1, 1, nt - 1);
#undef ROW
    pr->nplan = k;
    pr->p_len = ni + 3 + np;
    pr->n_trailing = nt;
    pr->pad_row = 3;
    return 0;
}

/* Voice clone (no c/ counterpart; the Python reference's layout,
 * modeling_qwen3_tts.py:2104-2232 + generate_icl_prompt :1967-2019; restated
 * by oracle/qtts_oracle.c orc_build_icl_prompt).  The speaker x-vector takes
 * the speaker-id slot (plan codec id -2); reference frames are plan codec ids
 * -3 - f (their 16 group embeddings summed on the device). */
typedef struct {
    const int *ref_ids;      /* ids of "<|im_start|>assistant\n{ref_text}<|im_end|>\n" (ICL) */
    int n_ref_ids;
    const int *ref_codes;    /* [n_ref][16] codes of the reference audio; NULL: x-vector only */
    int n_ref;
    const float *spk;        /* [hidden] speaker x-vector or NULL */
    int non_streaming;
} vclone_t;

static int build_icl_prompt(const qwen_tts_ctx_t *ctx, const int *ids, int n, const vclone_t *vc, int lang, int b,
                            prompt_t *pr) {
    const qwen_tts_config_t *c = &ctx->config;
    int prefix[8], np = 0;
    if (lang < 0) {
        prefix[np++] = c->codec_nothink_id; prefix[np++] = c->codec_think_bos_id; prefix[np++] = c->codec_think_eos_id;
    } else {
        prefix[np++] = c->codec_think_id; prefix[np++] = c->codec_think_bos_id; prefix[np++] = lang;
        prefix[np++] = c->codec_think_eos_id;
    }
    if (vc->spk) prefix[np++] = -2;
    prefix[np++] = c->codec_pad_id;
    prefix[np++] = c->codec_bos_id;
    const int icl = vc->ref_codes && vc->n_ref > 0;
    const int nr = icl && vc->n_ref_ids > 5 ? vc->n_ref_ids - 5 : 0, nx = n - 8 > 0 ? n - 8 : 0;
    /* text rows: 0-2 role, 3 pad, 4 bos, 5 eos, 6.. ref content ++ text content */
    /* (a plain-tail prompt of 8 ids still projects ids[3], as build_prompt does) */
    pr->n_text = 6 + nr + (!icl && nx == 0 ? 1 : nx);
    pr->text = (int *)malloc(pr->n_text * sizeof(int));
    int *t = pr->text;
    t[0] = ids[0]; t[1] = ids[1]; t[2] = ids[2];
    t[3] = QWEN_TTS_TOKEN_TTS_PAD; t[4] = QWEN_TTS_TOKEN_TTS_BOS; t[5] = QWEN_TTS_TOKEN_TTS_EOS;
    for (int i = 0; i < nr; i++) t[6 + i] = vc->ref_ids[3 + i];
    for (int i = 0; i < nx; i++) t[6 + nr + i] = ids[3 + i];
    if (!icl && nx == 0) t[6] = ids[3];
    const int Lt = nr + nx + 1, Lc = icl ? vc->n_ref + 1 : 0;
    pr->plan = (int *)malloc((size_t)(3 + np + 2 * (Lt + Lc) + 4) * 5 * sizeof(int));
    int k = 0, P = 0, nt = 0;
#define ROW(src, cid, kind, slot) do { int *r_ = pr->plan + 5 * k++; r_[0] = src; r_[1] = cid; r_[2] = kind; r_[3] = b; r_[4] = slot; } while (0)
#define TROW(j) ((j) < nr + nx ? 6 + (j) : 5)
#define CID(j) ((j) == 0 ? c->codec_bos_id : -3 - ((j) - 1))
    for (int i = 0; i < 3; i++) ROW(i, -1, 0, P++);
    for (int i = 0; i < np - 1; i++) ROW(i < np - 2 ? 3 : 4, prefix[i], 0, P++);
    if (!icl && !vc->non_streaming) {           /* x-vector only: the plain tail */
        ROW(6, c->codec_bos_id, 0, P++);        /* ids[3] = text row 6 */
        for (int j = 1; j < nx; j++) ROW(6 + j, -1, 1, nt++);
        ROW(5, -1, 1, nt++);
    } else if (!icl) {                          /* x-vector only, non-streaming (M.py:2203-2226) */
        for (int j = 0; j < Lt; j++) ROW(TROW(j), c->codec_pad_id, 0, P++);
        ROW(3, c->codec_bos_id, 0, P++);
        ROW(3, -1, 1, nt++);
    } else if (vc->non_streaming) {
        for (int j = 0; j < Lt; j++) ROW(TROW(j), c->codec_pad_id, 0, P++);
        for (int j = 0; j < Lc; j++) ROW(3, CID(j), 0, P++);
        ROW(3, -1, 1, nt++);
    } else {
        for (int j = 0; j < Lc; j++) ROW(j < Lt ? TROW(j) : 3, CID(j), 0, P++);
        if (Lt > Lc) for (int j = Lc; j < Lt; j++) ROW(TROW(j), -1, 1, nt++);
        else ROW(3, -1, 1, nt++);
    }
#undef CID
#undef TROW
#undef ROW
    pr->nplan = k;
    pr->p_len = P;
    pr->n_trailing = nt;
    pr->pad_row = 3;
    return 0;
}

static void lookup(const qwen_tts_ctx_t *ctx, const char *speaker, const char *language, int *spk, int *lang) {
    const qwen_tts_config_t *c = &ctx->config;
    *spk = -1;
    *lang = -1;
    if (speaker && strlen(speaker) > 0) {
        for (int i = 0; i < c->n_speakers; i++)
            if (strcasecmp(c->speaker_names[i], speaker) == 0) { *spk = c->speaker_ids[i]; break; }
        if (*spk < 0) fprintf(stderr, "Warning: speaker '%s' not found, using no speaker embedding\n", speaker);
    }
    if (language && strlen(language) > 0 && strcasecmp(language, "auto") != 0) {
        for (int i = 0; i < c->n_languages; i++)
            if (strcasecmp(c->language_names[i], language) == 0) { *lang = c->language_ids[i]; break; }
        if (*lang < 0) fprintf(stderr, "Warning: language '%s' not found\n", language);
    }
}

static int ids_in_range(const qwen_tts_ctx_t *ctx, const int *ids, int n) {
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= ctx->config.talker_text_vocab) {
            fprintf(stderr, "Error: text token id %d out of range\n", ids[i]);
            return 0;
        }
    return 1;
}

/* the reference text of an ICL voice: its ids (malloc'd) and their count, or -1 with the message */
static int ref_text_ids(const qwen_tts_ctx_t *ctx, const char *ref_text, int **ids) {
    *ids = NULL;
    const int n = ref_text ? parse_ids(ref_text, ids) : 0;
    if (n < 5) fprintf(stderr, "Error: ICL voice clone needs the reference text ids (chat template, >= 5 ids)\n");
    else if (ids_in_range(ctx, *ids, n)) return n;
    free(*ids);
    *ids = NULL;
    return -1;
}

/* Prompt intake of every generate path: one utterance's text ids, checked,
 * its speaker / language looked up, laid out for slot b (vc: the voice-clone
 * layout, the speaker name unused; ins / ni: the utterance's instruct ids,
 * preset-speaker and voice-design layouts only).  -1 with the message on a
 * refusal. */
static int prompt_make(const qwen_tts_ctx_t *ctx, const char *text, const char *speaker, const char *language,
                       const vclone_t *vc, const int *ins, int ni, int b, prompt_t *pr) {
    int *ids = NULL, rc = -1;
    const int n = parse_ids(text, &ids);
    if (n < 8) {
        if (n >= 0) fprintf(stderr, "Error: need at least 8 text tokens (chat template format)\n");
    } else if (ids_in_range(ctx, ids, n)) {
        int spk, lang;
        lookup(ctx, speaker, language, &spk, &lang);
        rc = vc ? build_icl_prompt(ctx, ids, n, vc, lang, b, pr) : build_prompt(ctx, ids, n, spk, lang, ins, ni, b, pr);
    }
    free(ids);
    return rc;
}

static void prompts_free(prompt_t *pr, int n) {
    for (int i = 0; pr && i < n; i++) { free(pr[i].text); free(pr[i].plan); }
    free(pr);
}

/* the reference codec's stderr lines around one full decode
 * (c/qwen_tts_codec.c:598-599 at -v, 740-746 at -v / -v -v) */
static void codec_log_begin(qwen_tts_ctx_t *ctx, int T) {
    qtts_dev_codec_timing((qtts_dev_t *)ctx->hip, qwen_tts_verbose >= 2);
    if (qwen_tts_verbose >= 1)
        fprintf(stderr, "Codec decode: %d timesteps, %d quantizers\n", T, ctx->config.codec_num_quantizers);
}

static void codec_log_end(qwen_tts_ctx_t *ctx, int samples) {
    if (qwen_tts_verbose < 1 || samples <= 0) return;
    fprintf(stderr, "Codec decode complete: %d samples (%.2f seconds)\n", samples,
            (float)samples / QWEN_TTS_SAMPLE_RATE);
    float ms[5];
    if (qwen_tts_verbose >= 2 && qtts_dev_codec_stage_ms((qtts_dev_t *)ctx->hip, ms) == 0)
        fprintf(stderr, "Codec stages (ms): rvq=%.1f preconv=%.1f transformer=%.1f upsample=%.1f vocoder=%.1f\n",
                ms[0], ms[1], ms[2], ms[3], ms[4]);
}

/* voice clone: keep the audio after the reference frames of a decode of
 * reference ++ generated codes (qwen3_tts_model.py:612-630, the same float
 * cut); takes ownership of w */
static void cut_reference(float *w, int nw, int n_ref, int tot, float **audio, int *samples) {
    const int cut = (int)((double)n_ref / (double)tot * (double)nw);
    *audio = NULL;
    *samples = 0;
    if (w && nw > cut) {
        memmove(w, w + cut, (size_t)(nw - cut) * sizeof(float));
        *audio = w;
        *samples = nw - cut;
    } else {
        free(w);
    }
}

static void params_of(const qwen_tts_ctx_t *ctx, qtts_gen_params_t *p) {
    p->temperature = ctx->temperature; p->top_p = ctx->top_p; p->repetition_penalty = ctx->repetition_penalty;
    p->top_k = ctx->top_k; p->st_temperature = ctx->subtalker_temperature; p->st_top_p = ctx->subtalker_top_p;
    p->st_top_k = ctx->subtalker_top_k; p->fixed_codec_tokens = ctx->fixed_codec_tokens; p->seed = ctx->sample_seed;
}

/* ------------------------------------------------ teacher forcing and taps */
/* What qwen_tts_force_codes / qwen_tts_tap_draw armed for the NEXT generation
 * call (ctx->force).  One-shot: run_batch detaches it on entry, so the call
 * consumes it whether it succeeds or not and a ctx shared between callers
 * cannot inherit it; the public entries that can fail before run_batch drop it
 * themselves (force_disarm). */
#define FORCE_MAX_TAPS 8
typedef struct {
    int slot, n_frames;
    int *codes;                  /* [n_frames][G], < 0 free */
} force_slot_t;
typedef struct {
    int n_slots;
    force_slot_t *slots;
    int n_taps;
    int taps[FORCE_MAX_TAPS][3]; /* slot, frame, group */
} force_arm_t;

static void force_free(force_arm_t *a) {
    if (!a) return;
    for (int i = 0; i < a->n_slots; i++) free(a->slots[i].codes);
    free(a->slots);
    free(a);
}

/* ------------------------------------------- per-utterance sampling (one-shot) */
/* What qwen_tts_set_utterance_sampling armed for the NEXT generation call
 * (ctx->sampling): detached on entry by run_batch / qwen_tts_generate_queue
 * (sampling_take), dropped with the forcing by every entry that fails before
 * them (force_disarm). */
typedef struct {
    int n;
    qwen_tts_sampling_t *per;   /* [n] */
} sampling_arm_t;

static void sampling_free(sampling_arm_t *a) {
    if (!a) return;
    free(a->per);
    free(a);
}

static sampling_arm_t *sampling_take(qwen_tts_ctx_t *ctx) {
    sampling_arm_t *a = (sampling_arm_t *)ctx->sampling;
    ctx->sampling = NULL;
    return a;
}

static int sampling_ok(const qwen_tts_sampling_t *s, int i) {
    const float f[5] = {s->temperature, s->top_p, s->repetition_penalty, s->subtalker_temperature, s->subtalker_top_p};
    for (int k = 0; k < 5; k++)
        if (!isfinite(f[k])) {
            fprintf(stderr, "Error: utterance sampling %d: a non-finite value\n", i);
            return 0;
        }
    if (s->top_p <= 0.0f || s->subtalker_top_p <= 0.0f || s->repetition_penalty <= 0.0f) {
        fprintf(stderr, "Error: utterance sampling %d: top_p %g / %g and repetition_penalty %g must be > 0\n", i,
                s->top_p, s->subtalker_top_p, s->repetition_penalty);
        return 0;
    }
    return 1;
}

int qwen_tts_sampling_defaults(const qwen_tts_ctx_t *ctx, qwen_tts_sampling_t *s) {
    if (!ctx || !ctx->hip || !s) return -1;
    s->temperature = ctx->temperature; s->top_p = ctx->top_p; s->repetition_penalty = ctx->repetition_penalty;
    s->top_k = ctx->top_k; s->subtalker_temperature = ctx->subtalker_temperature;
    s->subtalker_top_p = ctx->subtalker_top_p; s->subtalker_top_k = ctx->subtalker_top_k;
    s->sample_seed = ctx->sample_seed;
    return 0;
}

int qwen_tts_set_utterance_sampling(qwen_tts_ctx_t *ctx, int n, const qwen_tts_sampling_t *per) {
    if (!ctx || !ctx->hip) return -1;
    if (n < 1 || !per) {
        fprintf(stderr, "Error: utterance sampling: %d parameter sets\n", n);
        return -1;
    }
    for (int i = 0; i < n; i++)
        if (!sampling_ok(&per[i], i)) return -1;
    sampling_arm_t *a = (sampling_arm_t *)calloc(1, sizeof(sampling_arm_t));
    if (!a) return -1;
    a->per = (qwen_tts_sampling_t *)malloc((size_t)n * sizeof(qwen_tts_sampling_t));
    if (!a->per) { free(a); return -1; }
    memcpy(a->per, per, (size_t)n * sizeof(qwen_tts_sampling_t));
    a->n = n;
    sampling_free((sampling_arm_t *)ctx->sampling);   /* armed again: the later call replaces */
    ctx->sampling = a;
    return 0;
}

/* utterance u's row on slot b of the device (after qtts_dev_begin) */
static int sampling_apply(qtts_dev_t *dev, const sampling_arm_t *a, int u, int b) {
    const qwen_tts_sampling_t *s = &a->per[u];
    qtts_slot_params_t p;
    p.temperature = s->temperature; p.top_p = s->top_p; p.repetition_penalty = s->repetition_penalty;
    p.top_k = s->top_k; p.st_temperature = s->subtalker_temperature; p.st_top_p = s->subtalker_top_p;
    p.st_top_k = s->subtalker_top_k; p.seed = s->sample_seed;
    return qtts_dev_slot_params(dev, b, &p);
}

/* ------------------------------------------------- instruct (one-shot) */
/* What qwen_tts_set_utterance_instruct armed for the NEXT generation call
 * (ctx->instruct): utterance i's instruct ids (n_ids[i] 0: none), checked at
 * arming.  Detached on entry by run_batch / queue_run (instruct_take), dropped
 * with the other two armings by every entry that fails before them
 * (force_disarm). */
typedef struct {
    int n;
    int **ids;    /* [n] malloc'd id lists, NULL where none */
    int *n_ids;   /* [n] */
} instruct_arm_t;

static void instruct_free(instruct_arm_t *a) {
    if (!a) return;
    for (int i = 0; a->ids && i < a->n; i++) free(a->ids[i]);
    free(a->ids);
    free(a->n_ids);
    free(a);
}

static instruct_arm_t *instruct_take(qwen_tts_ctx_t *ctx) {
    instruct_arm_t *a = (instruct_arm_t *)ctx->instruct;
    ctx->instruct = NULL;
    return a;
}

int qwen_tts_set_utterance_instruct(qwen_tts_ctx_t *ctx, int n, const char *const *instruct_ids) {
    if (!ctx || !ctx->hip) return -1;
    if (n < 1 || !instruct_ids) {
        fprintf(stderr, "Error: utterance instruct: %d id lists\n", n);
        return -1;
    }
    instruct_arm_t *a = (instruct_arm_t *)calloc(1, sizeof(instruct_arm_t));
    if (!a) return -1;
    a->n = n;
    a->ids = (int **)calloc(n, sizeof(int *));
    a->n_ids = (int *)calloc(n, sizeof(int));
    if (!a->ids || !a->n_ids) { instruct_free(a); return -1; }
    for (int i = 0; i < n; i++) {
        if (!instruct_ids[i]) continue;   /* (NULL or empty: no instruct for utterance i) */
        const int k = parse_ids(instruct_ids[i], &a->ids[i]);
        if (k < 0 || !ids_in_range(ctx, a->ids[i], k)) {
            fprintf(stderr, "Error: utterance instruct %d refused\n", i);
            instruct_free(a);
            return -1;
        }
        a->n_ids[i] = k;
    }
    instruct_free((instruct_arm_t *)ctx->instruct);   /* armed again: the later call replaces */
    ctx->instruct = a;
    return 0;
}

/* the entry check of a generation call of `n` utterances: 0 to go on */
static int instruct_refused(const char *who, const instruct_arm_t *ia, int n, int voice_clone) {
    if (!ia) return 0;
    if (voice_clone) {
        fprintf(stderr, "Error: %s: an instruct is armed for a voice-clone call (not supported; disarmed)\n", who);
        return 1;
    }
    if (ia->n != n) {
        fprintf(stderr, "Error: %s: %d instructs armed for a call of %d utterances (disarmed)\n", who, ia->n, n);
        return 1;
    }
    return 0;
}

/* the entry checks of a generation call of `n` utterances: 0 to go on */
static int sampling_refused(const char *who, const sampling_arm_t *sa, const void *force, int n) {
    if (!sa) return 0;
    if (force) {
        fprintf(stderr, "Error: %s: per-utterance sampling and forced codes / taps are both armed "
                        "(not supported; both disarmed)\n", who);
        return 1;
    }
    if (sa->n != n) {
        fprintf(stderr, "Error: %s: %d utterance sampling sets armed for a call of %d utterances (disarmed)\n", who,
                sa->n, n);
        return 1;
    }
    return 0;
}

/* drops whatever is armed for the next call: forcing / taps, per-utterance
 * sampling and instruct (every entry that fails before its run consumes all) */
static void force_disarm(qwen_tts_ctx_t *ctx) {
    force_free((force_arm_t *)ctx->force);
    ctx->force = NULL;
    sampling_free(sampling_take(ctx));
    instruct_free(instruct_take(ctx));
}

/* a voice-clone entry with an instruct armed: refused at the door, everything disarmed */
static int instruct_refuses_clone(qwen_tts_ctx_t *ctx, const char *who) {
    if (!ctx || !ctx->instruct) return 0;
    instruct_refused(who, (const instruct_arm_t *)ctx->instruct, 0, 1);
    force_disarm(ctx);
    return 1;
}

static force_arm_t *force_pending(qwen_tts_ctx_t *ctx) {
    if (!ctx->force) ctx->force = calloc(1, sizeof(force_arm_t));
    return (force_arm_t *)ctx->force;
}

int qwen_tts_force_codes(qwen_tts_ctx_t *ctx, int slot, const int *codes, int n_frames) {
    if (!ctx || !ctx->hip) return -1;
    const qwen_tts_config_t *c = &ctx->config;
    const int G = c->num_code_groups;
    if (slot < 0 || n_frames < 0 || (n_frames > 0 && !codes)) {
        fprintf(stderr, "Error: forced codes: bad slot %d or frame count %d\n", slot, n_frames);
        return -1;
    }
    for (int f = 0; f < n_frames; f++)
        for (int g = 0; g < G; g++) {
            const int id = codes[(size_t)f * G + g];
            const int ok = id < 0 || (g == 0 ? (id < c->talker_vocab_size - 1024 || id == c->codec_eos_id) &&
                                                   id < c->talker_vocab_size
                                             : id < c->subtalker_vocab_size);
            if (!ok) {
                fprintf(stderr, "Error: forced code %d at frame %d, group %d is out of range\n", id, f, g);
                return -1;
            }
        }
    force_arm_t *a = force_pending(ctx);
    if (!a) return -1;
    force_slot_t *fs = NULL;
    for (int i = 0; i < a->n_slots; i++)
        if (a->slots[i].slot == slot) fs = &a->slots[i];   /* armed again: the later call replaces */
    if (!fs) {
        force_slot_t *ns = (force_slot_t *)realloc(a->slots, (size_t)(a->n_slots + 1) * sizeof(force_slot_t));
        if (!ns) return -1;
        a->slots = ns;
        fs = &a->slots[a->n_slots++];
        fs->slot = slot;
        fs->codes = NULL;
    }
    free(fs->codes);
    fs->n_frames = n_frames;
    fs->codes = (int *)malloc((size_t)(n_frames > 0 ? n_frames : 1) * G * sizeof(int));
    if (!fs->codes) { fs->n_frames = 0; return -1; }
    if (n_frames > 0) memcpy(fs->codes, codes, (size_t)n_frames * G * sizeof(int));
    return 0;
}

int qwen_tts_tap_draw(qwen_tts_ctx_t *ctx, int slot, int frame, int group) {
    if (!ctx || !ctx->hip) return -1;
    if (slot < 0 || frame < 0 || group < 0 || group >= ctx->config.num_code_groups) {
        fprintf(stderr, "Error: tap (slot %d, frame %d, group %d) is out of range\n", slot, frame, group);
        return -1;
    }
    force_arm_t *a = force_pending(ctx);
    if (!a) return -1;
    if (a->n_taps >= FORCE_MAX_TAPS) {
        fprintf(stderr, "Error: at most %d taps per run\n", FORCE_MAX_TAPS);
        return -1;
    }
    a->taps[a->n_taps][0] = slot; a->taps[a->n_taps][1] = frame; a->taps[a->n_taps][2] = group;
    return a->n_taps++;
}

/* Hands the arming to the device for a run of nb slots and max_tokens frames
 * (after qtts_dev_begin, before anything launches).  A slot >= nb, more forced
 * frames than max_tokens or a tap past them fails the call. */
static int force_apply(qtts_dev_t *dev, const force_arm_t *a, int nb, int max_tokens) {
    if (!a) return 0;
    for (int i = 0; i < a->n_slots; i++) {
        const force_slot_t *fs = &a->slots[i];
        if (fs->slot >= nb || fs->n_frames > max_tokens) {
            fprintf(stderr, "Error: forced codes for slot %d (%d frames) do not fit a run of %d slots, %d frames\n",
                    fs->slot, fs->n_frames, nb, max_tokens);
            return -1;
        }
    }
    for (int i = 0; i < a->n_taps; i++)
        if (a->taps[i][0] >= nb || a->taps[i][1] >= max_tokens) {
            fprintf(stderr, "Error: tap (slot %d, frame %d) does not fit a run of %d slots, %d frames\n",
                    a->taps[i][0], a->taps[i][1], nb, max_tokens);
            return -1;
        }
    for (int i = 0; i < a->n_slots; i++)
        if (qtts_dev_force(dev, a->slots[i].slot, a->slots[i].codes, a->slots[i].n_frames) != 0) return -1;
    for (int i = 0; i < a->n_taps; i++)
        if (qtts_dev_tap(dev, a->taps[i][0], a->taps[i][1], a->taps[i][2]) != i) return -1;
    return 0;
}

int qwen_tts_last_drawn(qwen_tts_ctx_t *ctx, int slot, int *codes, int max_frames) {
    if (!ctx || !ctx->hip || slot < 0 || !codes || max_frames < 0) return -1;
    return qtts_dev_get_drawn((qtts_dev_t *)ctx->hip, slot, codes, max_frames);
}

int qwen_tts_tap_result(qwen_tts_ctx_t *ctx, int i, float *logits, int max_n, unsigned *rng_bits, int *drawn) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_get_tap((qtts_dev_t *)ctx->hip, i, logits, max_n, rng_bits, drawn);
}

/* ------------------------------------------------------------- generation */
typedef struct {                 /* streaming arguments of a generate call */
    qwen_tts_audio_cb cb;        /* the single exact stream of one utterance */
    void *user;
    int chunk;
    int multi;                   /* every slot through the multi-stream codec, chunks to bcb */
    qwen_tts_batch_audio_cb bcb;
} stream_t;

/* Streaming delivery, shared by the lock-step run and the work queue: the
 * per-run state, and the one routine that pushes new frames through a codec
 * stream and hands the audio on.  The two loops differ only in how they decide
 * which slots are due (batch_flush, queue_flush). */
typedef struct {
    const stream_t *stream;
    int n;                       /* slots */
    float **buf;                 /* [n] the slot's utterance so far, max_tokens * 1920 samples each */
    int *done;                   /* [n] frames of it delivered */
    int *stream_of_slot;         /* [n] (the queue's tail compaction moves the entry, never codec state) */
    double t_stream, t_start;    /* time in the pushes / the first packet's origin */
    int delivered;               /* callbacks so far */
    int stamp_first_cb;          /* the queue: the first packet is stamped before the call's first callback
                                    (a lock-step run stamps it once its first flush is over: batch_flush) */
} sstate_t;

static void sstate_free(sstate_t *s) {
    for (int b = 0; s->buf && b < s->n; b++) free(s->buf[b]);
    free(s->buf); free(s->done); free(s->stream_of_slot);
    memset(s, 0, sizeof *s);
}

static int sstate_init(sstate_t *s, const stream_t *stream, int n, int max_tokens, double t_start, int stamp_first_cb) {
    memset(s, 0, sizeof *s);
    s->stream = stream;
    s->n = n;
    s->t_start = t_start;
    s->stamp_first_cb = stamp_first_cb;
    s->buf = (float **)calloc(n, sizeof(float *));
    s->done = (int *)calloc(n, sizeof(int));
    s->stream_of_slot = (int *)malloc(n * sizeof(int));
    int ok = s->buf && s->done && s->stream_of_slot;
    for (int b = 0; b < n && ok; b++) {
        s->stream_of_slot[b] = b;
        ok = (s->buf[b] = (float *)malloc((size_t)max_tokens * 1920 * sizeof(float))) != NULL;
    }
    return ok ? 0 : -1;
}

/* One push: slot slots[i]'s next cnt[i] frames (from done[slot] on) through
 * its stream, into its buffer; the time goes to t_stream, the queue's first
 * packet is stamped, every slot's callback gets the pointer into its buffer, its sample
 * count and utt[slot] (NULL: the slot index).  The entry: the single stream
 * for a non-multi call; _push_slots for slots at equal positions with equal
 * counts (!at_positions); else _push_slots_at, or _push_slots_ragged when the
 * counts differ. */
static int stream_deliver(qwen_tts_ctx_t *ctx, qtts_dev_t *dev, sstate_t *s, int n, const int *slots, const int *cnt,
                          int at_positions, const int *utt) {
    const stream_t *st = s->stream;
    int ids[QWEN_TTS_MAX_BATCH], f0[QWEN_TTS_MAX_BATCH], same = 1, r;
    float *outs[QWEN_TTS_MAX_BATCH];
    for (int i = 0; i < n; i++) {
        ids[i] = s->stream_of_slot[slots[i]];
        f0[i] = s->done[slots[i]];
        outs[i] = s->buf[slots[i]] + (size_t)f0[i] * 1920;
        same &= cnt[i] == cnt[0];
    }
    const double t0 = now_ms();
    if (!st->multi) r = qtts_dev_codec_stream_push_slot(dev, slots[0], f0[0], cnt[0], outs[0]);
    else if (!at_positions) r = qtts_dev_codec_mstream_push_slots(dev, n, ids, slots, f0[0], cnt[0], outs);
    else if (same) r = qtts_dev_codec_mstream_push_slots_at(dev, n, ids, slots, f0, cnt[0], outs);
    else r = qtts_dev_codec_mstream_push_slots_ragged(dev, n, ids, slots, f0, cnt, outs);
    if (r < 0) return -1;
    s->t_stream += now_ms() - t0;
    const int first = s->delivered == 0;
    for (int i = 0; i < n; i++) {
        if (first && i == 0 && s->stamp_first_cb) ctx->perf_first_packet_ms = now_ms() - s->t_start;
        if (!st->multi) { if (st->cb) st->cb(outs[i], r, st->user); }
        else if (st->bcb) st->bcb(utt ? utt[slots[i]] : slots[i], outs[i], same ? r : cnt[i] * 1920, st->user);
        s->done[slots[i]] += cnt[i];
    }
    s->delivered += n;
    return 0;
}

/* What a lock-step run delivers after a poll: every slot's new frames.  The
 * slots decode in lock step and a slot that stopped was brought up to date by
 * the poll that saw it stop, so every slot with new frames is at the same
 * position; they differ only in how many are new (a short tail): one push per
 * distinct count, in first-seen order.  at_positions (a voice-clone batch:
 * each stream stands at its primed reference frames + its own): one push for
 * all, whatever the counts.  The first packet is stamped when a flush that
 * began with nothing delivered is over: every slot then has its first chunk
 * (the single stream: only if it pushed). */
static int batch_flush(qwen_tts_ctx_t *ctx, qtts_dev_t *dev, sstate_t *s, const int *ngen, int at_positions) {
    int todo[QWEN_TTS_MAX_BATCH];
    const int first = s->delivered == 0;
    for (int b = 0; b < s->n; b++) todo[b] = ngen[b] - s->done[b];
    for (;;) {
        int n = 0, T = 0, slots[QWEN_TTS_MAX_BATCH], cnt[QWEN_TTS_MAX_BATCH];
        for (int b = 0; b < s->n; b++)
            if (todo[b] > 0 && (at_positions || !T || todo[b] == T)) {
                if (!T) T = todo[b];
                slots[n] = b;
                cnt[n++] = todo[b];
                todo[b] = 0;
            }
        if (!n) break;
        if (stream_deliver(ctx, dev, s, n, slots, cnt, at_positions, NULL) != 0) return -1;
    }
    if (first && (s->stream->multi || s->delivered)) ctx->perf_first_packet_ms = now_ms() - s->t_start;
    return 0;
}

/* The final codec pass of several utterances, side by side on the codec lanes
 * (qtts_dev_codec_multi).  Job j fills audio[utt] / samples[utt] from n_gen
 * generated frames: host `codes`, or (NULL) device slot `slot`'s.  An ICL
 * voice's job carries its reference codes: it decodes reference ++ generated
 * and keeps the part after the reference (cut_reference).  A job whose codes
 * cannot be put together, or that comes back without audio, leaves its output
 * NULL and makes the result -1; the others still decode.  log: the per-job -v
 * lines of a lock-step batch (the -v -v stage times are a lone decode's only:
 * the lanes run side by side). */
typedef struct {
    int utt, slot, n_gen;
    const int *codes;
    const int *ref;
    int n_ref;
} codec_job_t;

static int codec_finish(qwen_tts_ctx_t *ctx, qtts_dev_t *dev, int nj, const codec_job_t *jobs, int log,
                        float **audio, int *samples) {
    const int G = ctx->config.num_code_groups;
    const int **hc = (const int **)calloc(nj, sizeof(int *));
    int **own = (int **)calloc(nj, sizeof(int *));
    int *slot = (int *)calloc(nj, sizeof(int)), *T = (int *)calloc(nj, sizeof(int));
    int *of = (int *)calloc(nj, sizeof(int)), *sj = (int *)calloc(nj, sizeof(int));
    float **aj = (float **)calloc(nj, sizeof(float *));
    int n = 0, rc = hc && own && slot && T && of && sj && aj ? 0 : -1;
    for (int j = 0; j < nj && rc == 0; j++) {
        const codec_job_t *jb = &jobs[j];
        const int tot = jb->n_ref + jb->n_gen;
        hc[n] = jb->codes;
        if (jb->n_ref > 0) {
            int *all = (int *)malloc((size_t)tot * G * sizeof(int));
            if (!all) continue;   /* (the job has no audio: -1 below) */
            int *gen = all + (size_t)jb->n_ref * G;
            if (jb->codes) {
                memcpy(gen, jb->codes, (size_t)jb->n_gen * G * sizeof(int));
            } else if (qtts_dev_get_codes(dev, jb->slot, gen, jb->n_gen) != jb->n_gen) {
                free(all);
                continue;
            }
            memcpy(all, jb->ref, (size_t)jb->n_ref * G * sizeof(int));
            hc[n] = own[n] = all;
        }
        slot[n] = jb->slot;
        T[n] = tot;
        of[n] = j;
        if (log && qwen_tts_verbose >= 1)
            fprintf(stderr, "Codec decode: %d timesteps, %d quantizers\n", tot, ctx->config.codec_num_quantizers);
        n++;
    }
    if (rc == 0 && n < nj) rc = -1;
    if (n > 0 && qtts_dev_codec_multi(dev, n, hc, slot, T, aj, sj) != 0) rc = -1;
    for (int k = 0; k < n; k++) {
        const codec_job_t *jb = &jobs[of[k]];
        if (log && qwen_tts_verbose >= 1 && aj[k] && sj[k] > 0)
            fprintf(stderr, "Codec decode complete: %d samples (%.2f seconds)\n", sj[k],
                    (float)sj[k] / QWEN_TTS_SAMPLE_RATE);
        if (jb->n_ref > 0) {
            cut_reference(aj[k], sj[k], jb->n_ref, T[k], &audio[jb->utt], &samples[jb->utt]);
        } else {
            audio[jb->utt] = aj[k];
            samples[jb->utt] = aj[k] ? sj[k] : 0;
        }
        if (!audio[jb->utt] || samples[jb->utt] <= 0) rc = -1;
        free(own[k]);
    }
    free(hc); free(own); free(slot); free(T); free(of); free(sj); free(aj);
    return rc;
}

/* Runs nb utterances in lock-step frames.  Fills per-slot frame counts and
 * stop info; audio[i] decoded per slot.  Returns 0 on success. */
static int run_batch(qwen_tts_ctx_t *ctx, int nb, const char *const *texts, const char *const *speakers,
                     const char *const *languages, float **audio, int *samples, double t_start,
                     const stream_t *stream, const vclone_t *vcs /* [nb] or NULL */) {
    qtts_dev_t *dev = (qtts_dev_t *)ctx->hip;
    const qwen_tts_config_t *c = &ctx->config;
    const int G = c->num_code_groups;
    int rc = -1;
    force_arm_t *arm = (force_arm_t *)ctx->force;   /* one-shot: this call consumes it, however it ends */
    ctx->force = NULL;
    sampling_arm_t *sarm = sampling_take(ctx);      /* and the per-utterance sampling */
    instruct_arm_t *iarm = instruct_take(ctx);      /* and the instructs */
    /* what the run owns: freed at `out`, whichever way it is reached */
    prompt_t *pr = NULL;
    int *prime_codes = NULL;   /* the reference frames of a streamed voice-clone batch, kept until the run ends */
    int *stopped = NULL, *ngen = NULL, *sstep = NULL;
    codec_job_t *jobs = NULL;
    sstate_t ss;               /* streaming: exact incremental codec decode of the frames produced so far */
    memset(&ss, 0, sizeof ss);
    if (sampling_refused("generate", sarm, arm, nb) || instruct_refused("generate", iarm, nb, vcs != NULL)) goto out;
    if (!(pr = (prompt_t *)calloc(nb, sizeof(prompt_t)))) goto out;
    int max_p = 0;
    for (int b = 0; b < nb; b++) {
        if (prompt_make(ctx, texts[b], speakers ? speakers[b] : NULL, languages ? languages[b] : NULL,
                        vcs ? &vcs[b] : NULL, iarm ? iarm->ids[b] : NULL, iarm ? iarm->n_ids[b] : 0, b, &pr[b]) != 0)
            goto out;
        if (pr[b].p_len > max_p) max_p = pr[b].p_len;
    }
    const int fixed = ctx->fixed_codec_tokens > 0 ? ctx->fixed_codec_tokens : 0;
    const int max_tokens = fixed > 0 ? fixed : ctx->max_new_tokens;
    if (max_tokens < 1) goto out;
    qtts_gen_params_t gp;
    params_of(ctx, &gp);
    if (qtts_dev_begin(dev, nb, max_tokens, max_p, &gp) != 0) goto out;
    if (force_apply(dev, arm, nb, max_tokens) != 0) goto out;
    if (sarm)
        for (int b = 0; b < nb; b++)
            if (sampling_apply(dev, sarm, b, b) != 0) goto out;
    for (int b = 0; b < nb; b++)
        if ((vcs && qtts_dev_prompt_ref(dev, vcs[b].ref_codes, vcs[b].ref_codes ? vcs[b].n_ref : 0, vcs[b].spk) != 0) ||
            qtts_dev_prompt(dev, b, pr[b].text, pr[b].n_text, pr[b].plan, pr[b].nplan, pr[b].p_len,
                            pr[b].n_trailing, pr[b].pad_row) != 0)
            goto out;
    /* streaming voice clone: the reference frames go through the codec stream
     * first (their audio is dropped), so the carried codec state is that of
     * decoding reference ++ generated and the chunks start at the reference
     * boundary.  They run on a second HIP stream in one chunk while the
     * prefill runs (qtts_dev_codec_stream_prime); later pushes wait for them. */
    const int sref = stream && vcs && vcs[0].ref_codes && vcs[0].n_ref > 0 ? vcs[0].n_ref : 0;
    const int multi = stream && stream->multi;
    /* a streamed voice-clone batch: the same for every ICL slot, all their
     * reference frames in ONE ragged push of the multi-stream codec
     * (qtts_dev_codec_mstream_prime); an x-vector-only slot has none and its
     * stream stays at position 0 */
    if (multi && vcs) {
        int n = 0, ld = 0, ids[QWEN_TTS_MAX_BATCH], cnt[QWEN_TTS_MAX_BATCH];
        for (int b = 0; b < nb; b++) {
            const int nr = vcs[b].ref_codes && vcs[b].n_ref > 0 ? vcs[b].n_ref : 0;
            if (nr > ld) ld = nr;
            if (nr) { ids[n] = b; cnt[n++] = nr; }
        }
        if (qtts_dev_codec_mstream_begin(dev, nb, max_tokens + ld, 0) != 0) goto out;
        if (n) {
            prime_codes = (int *)calloc((size_t)n * ld * 16, sizeof(int));
            if (!prime_codes) goto out;
            for (int i = 0; i < n; i++)
                memcpy(prime_codes + (size_t)i * ld * 16, vcs[ids[i]].ref_codes, (size_t)cnt[i] * 16 * sizeof(int));
            if (qtts_dev_codec_mstream_prime(dev, n, ids, prime_codes, cnt, ld) != 0) goto out;
        }
    } else if (multi) {
        if (qtts_dev_codec_mstream_begin(dev, nb, max_tokens, 0) != 0) goto out;
    } else if (stream && (qtts_dev_codec_stream_begin_ex(dev, max_tokens + sref, sref) != 0 ||
                          (sref && qtts_dev_codec_stream_prime(dev, vcs[0].ref_codes, sref) != 0)))
        goto out;
    double t_prefill = now_ms();
    if (qtts_dev_prefill(dev) != 0) goto out;
    double t_prefill_done = now_ms();
    ctx->perf_prefill_ms = t_prefill_done - t_prefill;
    if (qwen_tts_verbose >= 1) {
        fprintf(stderr, "Talker prefill complete: %d tokens\n", pr[0].p_len);
        fprintf(stderr, "Prefill: %d tokens in %.1f ms\n", pr[0].p_len, t_prefill_done - t_prefill);
    }
    stopped = (int *)calloc(nb, sizeof(int));
    ngen = (int *)calloc(nb, sizeof(int));
    sstep = (int *)calloc(nb, sizeof(int));
    if (!stopped || !ngen || !sstep) goto out;
    if (stream && sstate_init(&ss, stream, nb, max_tokens, t_start, 0) != 0) goto out;
    const int at_positions = multi && vcs;
    int streamed = 0;   /* frames of the furthest slot delivered */
    double t_gen = now_ms();
    const int poll_every = fixed > 0 ? 0 : 8;
    /* EOS mode without streaming: a lagged poll per frame (qtts_dev_frame_done)
     * instead of a synchronous one every 8 frames */
    const int lagged = fixed == 0 && !stream;
    int step = 0;
    for (; step < max_tokens; step++) {
        if (qtts_dev_frame(dev, step) != 0) goto out;
        if (step == 0) {
            qtts_dev_poll(dev, NULL, NULL, NULL);
            ctx->perf_first_frame_ms = now_ms() - t_start;
        }
        if (ctx->progress_cb) ctx->progress_cb(step + 1, max_tokens, ctx->progress_cb_userdata);
        if (lagged) {   /* EOS mode: frame step is queued; stop once every slot had stopped by frame step - 1 */
            int done = 0;
            if (step >= 1 && qtts_dev_frame_done(dev, step - 1, &done) != 0) goto out;
            if (qwen_tts_verbose >= 1 && step > 0 && step % 10 == 0)
                fprintf(stderr, "\r  Token %d (%.1f ms/token)...", step, (now_ms() - t_gen) / step);
            if (done) break;
            continue;
        }
        const int want_stream = stream && (step == 0 || step + 1 - streamed >= stream->chunk || step + 1 == max_tokens);
        if (want_stream || (poll_every && ((step + 1) % poll_every == 0 || step + 1 == max_tokens))) {
            qtts_dev_poll(dev, stopped, ngen, sstep);
            if (stream) {
                if (batch_flush(ctx, dev, &ss, ngen, at_positions) != 0) goto out;
                for (int b = 0; b < nb; b++)
                    if (ss.done[b] > streamed) streamed = ss.done[b];
            }
            int all = 1;
            for (int b = 0; b < nb; b++) all &= stopped[b];
            if (qwen_tts_verbose >= 1 && ngen[0] > 0 && ngen[0] % 10 < poll_every)
                fprintf(stderr, "\r  Token %d (%.1f ms/token)...", ngen[0], (now_ms() - t_gen) / ngen[0]);
            if (all) break;
        }
    }
    qtts_dev_poll(dev, stopped, ngen, sstep);
    if (stream && batch_flush(ctx, dev, &ss, ngen, at_positions) != 0) goto out;
    double t_gen_done = now_ms();
    ctx->perf_talker_ms = t_gen_done - t_gen - ss.t_stream;
    ctx->perf_codec_tokens = ngen[0];
    ctx->last_stop_reason = stopped[0] ? 1 : 2;
    ctx->last_stop_step = stopped[0] ? sstep[0] : max_tokens;
    free(ctx->last_codes);
    ctx->last_codes = (int *)malloc((size_t)(ngen[0] > 0 ? ngen[0] : 1) * G * sizeof(int));
    ctx->last_frames = ngen[0] > 0 && ctx->last_codes ? qtts_dev_get_codes(dev, 0, ctx->last_codes, ngen[0]) : 0;
    if (ctx->last_frames < 0) ctx->last_frames = 0;   /* (codes that could not be read: none, not a negative count) */
    if (qwen_tts_verbose >= 1) {
        if (stopped[0]) fprintf(stderr, "EOS at step %d\n", sstep[0]);
        fprintf(stderr, "\r                                        \r");
        fprintf(stderr, "Generated %d codec tokens in %.1f ms (%.1f ms/token)\n", ngen[0], ctx->perf_talker_ms,
                ngen[0] > 0 ? ctx->perf_talker_ms / ngen[0] : 0);
        fprintf(stderr, "Stop: %s at step %d\n", stopped[0] ? "eos" : "max_tokens", ctx->last_stop_step);
        if (qwen_tts_verbose >= 2) {
            fprintf(stderr, "Token trace:");
            for (int i = 0; i < ctx->last_frames; i++)
                fprintf(stderr, "%s%d", i == 0 ? " " : ",", ctx->last_codes[(size_t)i * G]);
            fprintf(stderr, "\n");
        }
    }
    double t_codec = now_ms();
    rc = 0;
    if (stream) {   /* each slot's chunks already are its utterance: the buffer goes to the caller */
        for (int b = 0; b < nb; b++) {
            audio[b] = ss.buf[b];
            ss.buf[b] = NULL;
            samples[b] = ss.done[b] * 1920;
            if (ss.done[b] <= 0) { free(audio[b]); audio[b] = NULL; rc = -1; }
        }
        ctx->perf_codec_ms = ss.t_stream;
    } else if (nb == 1) {
        audio[0] = NULL;
        samples[0] = 0;
        if (ngen[0] <= 0) {
            rc = -1;
        } else if (vcs && vcs[0].ref_codes && vcs[0].n_ref > 0) {
            /* voice clone: decode reference ++ generated codes, keep the part
             * after the reference (qwen3_tts_model.py:612-630, same float cut) */
            const vclone_t *vc = &vcs[0];
            const int tot = vc->n_ref + ngen[0];
            int *all = (int *)malloc((size_t)tot * G * sizeof(int)), nw = 0;
            if (all && qtts_dev_get_codes(dev, 0, all + (size_t)vc->n_ref * G, ngen[0]) == ngen[0]) {
                memcpy(all, vc->ref_codes, (size_t)vc->n_ref * G * sizeof(int));
                codec_log_begin(ctx, tot);
                float *w = qtts_dev_codec_decode_host(dev, all, tot, &nw);
                codec_log_end(ctx, w ? nw : 0);
                cut_reference(w, nw, vc->n_ref, tot, &audio[0], &samples[0]);
            }
            free(all);
            if (!audio[0]) rc = -1;
        } else {
            codec_log_begin(ctx, ngen[0]);
            audio[0] = qtts_dev_codec_slot(dev, 0, ngen[0], &samples[0]);
            codec_log_end(ctx, audio[0] ? samples[0] : 0);
            if (!audio[0] || samples[0] <= 0) rc = -1;
        }
    } else {
        /* a batch: every slot's codec pass in one call (codec_finish); a slot
         * without frames gets no audio and makes the call return -1 */
        int nj = 0;
        for (int b = 0; b < nb; b++) {
            audio[b] = NULL;
            samples[b] = 0;
        }
        if (!(jobs = (codec_job_t *)calloc(nb, sizeof(codec_job_t)))) rc = -1;
        for (int b = 0; b < nb && jobs; b++) {
            if (ngen[b] <= 0) { rc = -1; continue; }
            const int icl = vcs && vcs[b].ref_codes && vcs[b].n_ref > 0;
            const codec_job_t jb = {b, b, ngen[b], NULL, icl ? vcs[b].ref_codes : NULL, icl ? vcs[b].n_ref : 0};
            jobs[nj++] = jb;
        }
        if (nj > 0 && codec_finish(ctx, dev, nj, jobs, 1, audio, samples) != 0) rc = -1;
    }
    if (!stream) {
        ctx->perf_codec_ms = now_ms() - t_codec;
    }
    ctx->perf_total_ms = now_ms() - t_start;
out:
    force_free(arm);
    sampling_free(sarm);
    instruct_free(iarm);
    free(prime_codes);
    free(stopped); free(ngen); free(sstep);
    free(jobs);
    sstate_free(&ss);
    prompts_free(pr, nb);
    return rc;
}

/* how every single-utterance entry ends: the one output of its batch form, or NULL */
static float *one_result(int rc, float *audio, int n, int *out_samples) {
    *out_samples = 0;
    if (rc != 0 || !audio || n <= 0) {
        free(audio);
        return NULL;
    }
    *out_samples = n;
    return audio;
}

/* the -v lines that end a call of n utterances: streamed: the first packet
 * first; batch: the audio summed over the utterances */
static void log_totals(const qwen_tts_ctx_t *ctx, int streamed, int batch, int n, const int *samples) {
    if (qwen_tts_verbose < 1) return;
    if (streamed) fprintf(stderr, "First packet: %.1f ms\n", ctx->perf_first_packet_ms);
    if (!batch) {
        fprintf(stderr, "Total: %.1f ms (%.2f s audio, %.2fx realtime)\n", ctx->perf_total_ms,
                (float)samples[0] / QWEN_TTS_SAMPLE_RATE,
                ((float)samples[0] / QWEN_TTS_SAMPLE_RATE) / (ctx->perf_total_ms / 1000.0));
        return;
    }
    double secs = 0;
    for (int i = 0; i < n; i++) secs += (double)samples[i] / QWEN_TTS_SAMPLE_RATE;
    fprintf(stderr, "Total: %.1f ms (%.2f s audio over %d utterances, %.2fx realtime)\n", ctx->perf_total_ms, secs, n,
            secs / (ctx->perf_total_ms / 1000.0));
}

float *qwen_tts_generate(qwen_tts_ctx_t *ctx, const char *text, const char *speaker, const char *language,
                         int *out_samples) {
    if (!ctx || !out_samples) return NULL;
    *out_samples = 0;
    double t_start = now_ms();
    float *audio = NULL;
    int n = 0;
    const char *texts[1] = {text}, *spk[1] = {speaker}, *lang[1] = {language};
    const int rc = run_batch(ctx, 1, texts, spk, lang, &audio, &n, t_start, NULL, NULL);
    audio = one_result(rc, audio, n, out_samples);
    if (audio && qwen_tts_verbose >= 1) fprintf(stderr, "Codec decode: %d samples in %.1f ms\n", n, ctx->perf_codec_ms);
    if (audio) log_totals(ctx, 0, 0, 1, &n);
    return audio;
}

/* more lock-step slots than a ctx runs: refused at the door (an arming is
 * consumed as by every failed call) */
static int batch_refused(qwen_tts_ctx_t *ctx, const char *who, int nb) {
    if (nb <= QWEN_TTS_MAX_BATCH) return 0;
    fprintf(stderr, "Error: %s: %d slots, at most %d per context\n", who, nb, QWEN_TTS_MAX_BATCH);
    force_disarm(ctx);
    return 1;
}

int qwen_tts_generate_batch(qwen_tts_ctx_t *ctx, int nb, const char *const *texts, const char *const *speakers,
                            const char *const *languages, float **out_audio, int *out_samples) {
    if (!ctx || nb < 1 || !texts || !out_audio || !out_samples) return -1;
    if (batch_refused(ctx, "qwen_tts_generate_batch", nb)) return -1;
    return run_batch(ctx, nb, texts, speakers, languages, out_audio, out_samples, now_ms(), NULL, NULL);
}

/* ------------------------------------------------------------- work queue */
/* EOS-mode utterances (Q.c:1282-1330: each stops at its own
 * EOS) on `nb` lock-step slots.  When a slot's utterance stops, its codes are
 * collected and the next queued utterance is prefilled into that slot inside
 * the live batch (qtts_dev_refill), so no slot rides along stopped while
 * others decode, except for the one frame the lagged stop poll costs.  The
 * frame loop is run_batch's: frame s + 1 is queued before the host waits for
 * frame s.  Every utterance decodes exactly as it would alone (its own KV
 * positions from 0, counters, repetition counts and RNG states from the seed);
 * the codec passes of all of them run at the end on the codec lanes
 * (qtts_dev_codec_multi). */
static int queue_pull(int nq, int *taken, int *next_seq, qwen_tts_queue_next_cb next, void *user) {
    if (next) {
        const int i = next(user);
        if (i < 0 || i >= nq || taken[i]) return -1;
        taken[i] = 1;
        return i;
    }
    while (*next_seq < nq && taken[*next_seq]) (*next_seq)++;
    if (*next_seq >= nq) return -1;
    taken[*next_seq] = 1;
    return (*next_seq)++;
}

static void queue_plan_slot(prompt_t *p, int b) {
    for (int k = 0; k < p->nplan; k++) p->plan[5 * k + 3] = b;
}

/* The streaming queue (stream != NULL; qwen_tts_generate_queue_stream): every
 * slot's frames go through a multi-stream codec stream of its own as they are
 * decoded (sstate_t).  Slot b's stream is stream_of_slot[b]: a refill resets it,
 * the tail compaction moves the map entry, never codec state.  After the wait for
 * frame step - 1, slot b has avail = min(step - first[b], its frame count if
 * it stopped) finished frames, done[b] of them delivered.  A slot is due when
 * it has delivered nothing and has a frame (the first packet: one frame), when
 * its utterance is complete (the tail: everything, before the slot's codes
 * rows are reused), or at the call's cadence (step % chunk == 0); the due
 * slots go in one push per distinct frame count, whatever their positions
 * (stream_deliver; the callback gets the utterance's index cur[slot]). */
static int queue_flush(qwen_tts_ctx_t *ctx, qtts_dev_t *dev, sstate_t *s, const int *cur, const int *avail,
                       const int *complete, int cadence) {
    for (;;) {
        int n = 0, T = 0, slots[QWEN_TTS_MAX_BATCH], cnt[QWEN_TTS_MAX_BATCH];
        for (int b = 0; b < s->n; b++) {
            int todo = 0;
            if (cur[b] < 0 || avail[b] <= s->done[b]) continue;
            if (s->done[b] == 0) todo = 1;
            else if (complete[b] || cadence) todo = avail[b] - s->done[b];
            if (todo > 0 && !T) T = todo;
            if (todo > 0 && todo == T) { slots[n] = b; cnt[n++] = T; }
        }
        if (!n) return 0;
        if (stream_deliver(ctx, dev, s, n, slots, cnt, 1, cur) != 0) return -1;
    }
}

/* A voice handle (qwen_tts_voice_*): a cloned voice's prompt inputs, copied,
 * and for an ICL voice the codec snapshot of its reference frames, made by
 * the first streamed call that uses the handle */
struct qwen_tts_voice {
    qwen_tts_ctx_t *ctx;             /* the context that made it, and that context's device */
    void *hip;
    int *ref_ids, n_ref_ids;         /* ICL: ids of the reference text's chat template */
    int *ref_codes, n_ref;           /* [n_ref][16]; NULL / 0: x-vector only */
    float *spk;                      /* [hidden] or NULL */
    qtts_codec_snapshot_t *snap;     /* the primed reference frames, or NULL */
};

static int voice_primed(const qwen_tts_voice_t *v) {
    return v->snap && qtts_dev_codec_snapshot_pos(v->snap) == v->n_ref;
}

/* The streamed voice queue's priming: every distinct ICL voice of the call
 * that has no snapshot yet goes through the codec streams once, at most ns
 * voices at a time in one ragged push with the audio dropped, is saved, and
 * the streams are reset.  Leaves every stream at position 0. */
static int voices_prime(qtts_dev_t *dev, int nq, const qwen_tts_voice_t *const *voices, int ns, int max_ref,
                        int **codes_keep /* the staged reference frames: the caller frees them when the run ends */) {
    qwen_tts_voice_t **todo = (qwen_tts_voice_t **)calloc(nq, sizeof(*todo));
    int nt = 0, rc = todo ? 0 : -1;
    for (int i = 0; i < nq && todo; i++) {
        qwen_tts_voice_t *v = (qwen_tts_voice_t *)voices[i];   /* (the handle gains its snapshot here) */
        int seen = v->n_ref <= 0 || voice_primed(v);
        for (int k = 0; k < nt && !seen; k++) seen = todo[k] == v;
        if (seen) continue;
        if (v->snap) {   /* a dead one (its context's state is gone): make it again */
            qtts_dev_codec_snapshot_free(v->snap);
            v->snap = NULL;
        }
        todo[nt++] = v;
    }
    int *codes = nt > 0 ? (int *)calloc((size_t)nt * max_ref * 16, sizeof(int)) : NULL;
    *codes_keep = codes;
    if (nt > 0 && !codes) rc = -1;
    for (int g = 0; g < nt && rc == 0; g += ns) {
        const int n = nt - g < ns ? nt - g : ns;
        int ids[QWEN_TTS_MAX_BATCH], cnt[QWEN_TTS_MAX_BATCH];
        int *gc = codes + (size_t)g * max_ref * 16;
        for (int k = 0; k < n; k++) {
            ids[k] = k;
            cnt[k] = todo[g + k]->n_ref;
            memcpy(gc + (size_t)k * max_ref * 16, todo[g + k]->ref_codes, (size_t)cnt[k] * 16 * sizeof(int));
        }
        if (qtts_dev_codec_mstream_prime(dev, n, ids, gc, cnt, max_ref) != 0) rc = -1;
        for (int k = 0; k < n && rc == 0; k++)
            if (!(todo[g + k]->snap = qtts_dev_codec_mstream_save(dev, k)) ||
                qtts_dev_codec_mstream_reset(dev, k) != 0)
                rc = -1;
    }
    free(todo);
    return rc;
}

/* an admission of the streamed voice queue: the slot's stream from the
 * voice's primed state (an x-vector-only voice: from position 0) */
static int voice_admit(qtts_dev_t *dev, int stream, const qwen_tts_voice_t *v) {
    if (qtts_dev_codec_mstream_reset(dev, stream) != 0) return -1;
    return v->n_ref > 0 ? qtts_dev_codec_mstream_restore(dev, stream, v->snap) : 0;
}

static int queue_run(qwen_tts_ctx_t *ctx, const char *who, int nq, const char *const *texts,
                     const char *const *speakers, const char *const *languages, int nb, qwen_tts_queue_next_cb next,
                     void *user, float **out_audio, int *out_samples, const stream_t *stream,
                     const qwen_tts_voice_t *const *voices /* NULL: preset speakers */, int non_streaming) {
    if (ctx && ctx->force) {   /* forcing is defined for one utterance per slot, not for the queue */
        fprintf(stderr, "Error: %s: forced codes / taps are armed (not supported; disarmed)\n", who);
        force_disarm(ctx);
        return -1;
    }
    if (!ctx || !ctx->hip || nq < 1 || nb < 1 || !texts || !out_audio || !out_samples) {
        if (ctx) force_disarm(ctx);
        return -1;
    }
    if (batch_refused(ctx, who, nb)) return -1;
    sampling_arm_t *sarm = sampling_take(ctx);   /* one-shot: this call consumes it, however it ends */
    instruct_arm_t *iarm = instruct_take(ctx);   /* (indexed by input order, like the sampling sets) */
    if (sampling_refused(who, sarm, NULL, nq) || instruct_refused(who, iarm, nq, voices != NULL)) {
        sampling_free(sarm);
        instruct_free(iarm);
        return -1;
    }
    for (int i = 0; voices && i < nq; i++) {
        if (voices[i] && voices[i]->ctx == ctx && voices[i]->hip == ctx->hip) continue;
        fprintf(stderr, "Error: %s: utterance %d: %s\n", who, i,
                voices[i] ? "the voice handle belongs to another context" : "no voice handle (NULL)");
        sampling_free(sarm);
        instruct_free(iarm);
        return -1;
    }
    qtts_dev_t *dev = (qtts_dev_t *)ctx->hip;
    const qwen_tts_config_t *c = &ctx->config;
    const int G = c->num_code_groups;
    const double t_start = now_ms();
    int rc = -1;
    queue_clear(ctx);
    for (int i = 0; i < nq; i++) { out_audio[i] = NULL; out_samples[i] = 0; }
    prompt_t *pr = (prompt_t *)calloc(nq, sizeof(prompt_t));
    int *taken = (int *)calloc(nq, sizeof(int)), next_seq = 0;
    ctx->queue_codes = (int **)calloc(nq, sizeof(int *));
    ctx->queue_frames = (int *)malloc(nq * sizeof(int));
    ctx->queue_stop_reason = (int *)calloc(nq, sizeof(int));
    ctx->queue_slot = (int *)malloc(nq * sizeof(int));
    int *cur = (int *)malloc(nb * sizeof(int)), *first = (int *)calloc(nb, sizeof(int));
    int *retired = (int *)calloc(nb, sizeof(int)), *hst = (int *)calloc(nb, sizeof(int));
    int *cbuf = NULL;
    sstate_t qs;
    memset(&qs, 0, sizeof qs);
    codec_job_t *jobs = NULL;
    int *avail = NULL, *complete = NULL, *ngen = NULL, finished = 0;
    /* the voice queue: utterance i's prompt inputs, from its handle */
    vclone_t *vcs = voices ? (vclone_t *)calloc(nq, sizeof(vclone_t)) : NULL;
    int *prime_codes = NULL, max_ref = 0;
    if (!pr || !taken || !ctx->queue_codes || !ctx->queue_frames || !ctx->queue_stop_reason || !ctx->queue_slot ||
        !cur || !first || !retired || !hst || (voices && !vcs))
        goto out;
    for (int i = 0; voices && i < nq; i++) {
        const qwen_tts_voice_t *v = voices[i];
        vcs[i].ref_ids = v->ref_ids; vcs[i].n_ref_ids = v->n_ref_ids;
        vcs[i].ref_codes = v->n_ref > 0 ? v->ref_codes : NULL; vcs[i].n_ref = v->n_ref > 0 ? v->n_ref : 0;
        vcs[i].spk = v->spk;
        vcs[i].non_streaming = non_streaming;
        if (vcs[i].n_ref > max_ref) max_ref = vcs[i].n_ref;
    }
    ctx->queue_n = nq;
    for (int i = 0; i < nq; i++) { ctx->queue_frames[i] = -1; ctx->queue_slot[i] = -1; }
    /* every prompt up front (the prefill and trailing capacities cover all) */
    int max_p = 0, max_tr = 0;
    for (int i = 0; i < nq; i++) {
        if (prompt_make(ctx, texts[i], speakers ? speakers[i] : NULL, languages ? languages[i] : NULL,
                        vcs ? &vcs[i] : NULL, iarm ? iarm->ids[i] : NULL, iarm ? iarm->n_ids[i] : 0, 0, &pr[i]) != 0)
            goto out;
        if (pr[i].p_len > max_p) max_p = pr[i].p_len;
        if (pr[i].n_trailing > max_tr) max_tr = pr[i].n_trailing;
    }
    const int fixed = ctx->fixed_codec_tokens > 0 ? ctx->fixed_codec_tokens : 0;
    const int max_tokens = fixed > 0 ? fixed : ctx->max_new_tokens;
    if (max_tokens < 1) goto out;
    /* the first nb utterances fill the slots */
    int ns = 0;
    while (ns < nb) {
        const int u = queue_pull(nq, taken, &next_seq, next, user);
        if (u < 0) break;
        cur[ns++] = u;
    }
    ctx->queue_slots = ns;
    if (ns == 0) { rc = 0; goto out; }   /* (another puller took everything) */
    qtts_gen_params_t gp;
    params_of(ctx, &gp);
    if (qtts_dev_begin(dev, ns, max_tokens, max_p, &gp) != 0 || qtts_dev_reserve(dev, max_tr) != 0) goto out;
    if (stream) {
        /* (voices: a stream stands at its reference frames + its own; the
         * voices without a snapshot are primed and saved once, here) */
        if (qtts_dev_codec_mstream_begin(dev, ns, max_tokens + max_ref, 0) != 0) goto out;
        if (voices && voices_prime(dev, nq, voices, ns, max_ref, &prime_codes) != 0) goto out;
        avail = (int *)calloc(ns, sizeof(int));
        complete = (int *)calloc(ns, sizeof(int));
        ngen = (int *)calloc(ns, sizeof(int));
        if (sstate_init(&qs, stream, ns, max_tokens, t_start, 1) != 0 || !avail || !complete || !ngen) goto out;
    }
    /* (a plan row's 4th int is the destination slot: set when the slot is known) */
    /* (the admitted utterance's sampling row goes in with its prompt: before
     * the initial prefill and before every qtts_dev_refill) */
    /* (a voice's reference codes and x-vector go in before its prompt, which consumes them) */
#define PROMPT(b, u) (queue_plan_slot(&pr[u], (b)), \
                      (sarm && sampling_apply(dev, sarm, (u), (b)) != 0) ? -1 : \
                      (vcs && qtts_dev_prompt_ref(dev, vcs[u].ref_codes, vcs[u].n_ref, vcs[u].spk) != 0) ? -1 : \
                      qtts_dev_prompt(dev, (b), pr[u].text, pr[u].n_text, pr[u].plan, pr[u].nplan, pr[u].p_len, \
                                      pr[u].n_trailing, pr[u].pad_row))
    for (int b = 0; b < ns; b++)
        if (PROMPT(b, cur[b]) != 0 || (stream && voices && voice_admit(dev, qs.stream_of_slot[b], voices[cur[b]]) != 0))
            goto out;
    double t_prefill = now_ms();
    if (qtts_dev_prefill(dev) != 0) goto out;
    ctx->perf_prefill_ms = now_ms() - t_prefill;
    cbuf = (int *)malloc((size_t)(max_tokens + 1) * G * sizeof(int));
    if (!cbuf) goto out;
    int active = ns, done_n = 0, rows = ns, exhausted = 0;
    /* tail compaction (nothing left to admit): the running slots move to the
     * first rows and the frames launch those only (QTTS_QUEUE_COMPACT=0: off) */
    const char *ce = getenv("QTTS_QUEUE_COMPACT");
    const int compact = !(ce && !strcmp(ce, "0"));
    int step = 0;
    const double t_gen = now_ms();
    for (;; step++) {
        /* a slot whose utterance produced max_tokens frames by frame step - 1
         * stops before frame step (host count: no EOS draw marks it) */
        for (int b = 0; b < ns; b++)
            if (cur[b] >= 0 && !retired[b] && step - first[b] >= max_tokens) {
                if (qtts_dev_retire(dev, b) != 0) goto out;
                retired[b] = 1;
            }
        if (qtts_dev_frame(dev, step) != 0) goto out;
        ctx->queue_rows_launched += rows;
        if (step == 0) {
            qtts_dev_poll(dev, NULL, NULL, NULL);
            ctx->perf_first_frame_ms = now_ms() - t_start;
        }
        if (step < 1) continue;
        /* frame step is queued: which slots had stopped by frame step - 1 */
        if (qtts_dev_frame_stops(dev, step - 1, hst) != 0) goto out;
        if (stream) {
            /* what every slot has finished by frame step - 1, and the due slots' pushes:
             * before a complete slot's codes rows are reused or moved below */
            int any_complete = 0;
            for (int b = 0; b < ns; b++) {
                complete[b] = cur[b] >= 0 && (hst[b] || step - first[b] >= max_tokens);
                any_complete |= complete[b];
            }
            if (any_complete && qtts_dev_poll(dev, NULL, ngen, NULL) != 0) goto out;
            const int cadence = step % stream->chunk == 0;
            for (int b = 0; b < ns; b++) {
                avail[b] = cur[b] < 0 ? 0 : complete[b] ? ngen[b] : step - first[b];
                if (avail[b] > max_tokens) avail[b] = max_tokens;
            }
            if (queue_flush(ctx, dev, &qs, cur, avail, complete, cadence) != 0) goto out;
        }
        for (int b = 0; b < ns; b++) {
            if (cur[b] < 0) continue;
            const int capped = step - first[b] >= max_tokens;
            if (!hst[b] && !capped) continue;
            /* utterance cur[b] is complete (slot b is a no-op in frame step) */
            const int u = cur[b];
            const int n = qtts_dev_get_codes(dev, b, cbuf, max_tokens);
            if (n < 0) goto out;
            ctx->queue_codes[u] = (int *)malloc((size_t)(n > 0 ? n : 1) * G * sizeof(int));
            if (!ctx->queue_codes[u]) goto out;
            memcpy(ctx->queue_codes[u], cbuf, (size_t)n * G * sizeof(int));
            ctx->queue_frames[u] = n;
            ctx->queue_stop_reason[u] = hst[b] ? 1 : 2;
            ctx->queue_slot[u] = b;
            ctx->queue_slot_frames_used += n;
            done_n++;
            if (qwen_tts_verbose >= 1)
                fprintf(stderr, "Queue: utterance %d on slot %d: %s at step %d (frame %d)\n", u, b,
                        hst[b] ? "eos" : "max_tokens", n, step - 1);
            if (stream) {   /* its chunks already are the utterance (flushed above) */
                if (qs.done[b] != n) goto out;
                if (n > 0) {
                    if (!(out_audio[u] = (float *)malloc((size_t)n * 1920 * sizeof(float)))) goto out;
                    memcpy(out_audio[u], qs.buf[b], (size_t)n * 1920 * sizeof(float));
                    out_samples[u] = n * 1920;
                }
                qs.done[b] = 0;
            }
            cur[b] = -1;
            active--;
            const int u2 = exhausted ? -1 : queue_pull(nq, taken, &next_seq, next, user);
            if (u2 < 0) { exhausted = 1; continue; }
            if (stream && (voices ? voice_admit(dev, qs.stream_of_slot[b], voices[u2])
                                  : qtts_dev_codec_mstream_reset(dev, qs.stream_of_slot[b])) != 0)
                goto out;
            if (PROMPT(b, u2) != 0 || qtts_dev_refill(dev, b) != 0) goto out;
            cur[b] = u2;
            first[b] = step + 1;   /* its frame 0 is the next frame launched */
            retired[b] = 0;
            hst[b] = 0;
            active++;
            ctx->queue_refills++;
        }
        if (active == 0) break;
        if (exhausted && compact && active < rows) {
            /* every freed slot below the last running one takes that one's state */
            for (int i = 0; i < rows; i++) {
                if (cur[i] >= 0) continue;
                int j = rows - 1;
                while (j > i && cur[j] < 0) j--;
                if (j <= i) break;
                if (qtts_dev_move_slot(dev, j, i) != 0) goto out;
                cur[i] = cur[j]; first[i] = first[j]; retired[i] = retired[j];
                cur[j] = -1;
                if (stream) {   /* the slot's stream, frames delivered and chunk buffer travel with it */
                    const int sw = qs.stream_of_slot[i];
                    float *bw = qs.buf[i];
                    qs.stream_of_slot[i] = qs.stream_of_slot[j]; qs.stream_of_slot[j] = sw;
                    qs.buf[i] = qs.buf[j]; qs.buf[j] = bw;
                    qs.done[i] = qs.done[j]; qs.done[j] = 0;
                }
            }
            rows = active;
            if (qtts_dev_set_rows(dev, rows) != 0) goto out;
        }
        if (ctx->progress_cb) ctx->progress_cb(done_n, nq, ctx->progress_cb_userdata);
    }
#undef PROMPT
    ctx->queue_frames_launched = step + 1;
    ctx->perf_talker_ms = now_ms() - t_gen - qs.t_stream;
    if (stream) {
        rc = 0;
        finished = 1;
        for (int u = 0; u < nq; u++)
            if (ctx->queue_frames[u] == 0) rc = -1;   /* (taken, no frame: no audio) */
        ctx->perf_codec_ms = qs.t_stream;
    } else {
        /* every finished utterance's codec pass from its collected codes
         * (codec_finish; an ICL voice's with its reference codes ahead) */
        int nj = 0;
        if (!(jobs = (codec_job_t *)calloc(nq, sizeof(codec_job_t)))) goto out;
        rc = 0;
        for (int u = 0; u < nq; u++) {
            if (ctx->queue_frames[u] < 0) continue;   /* not taken by this ctx */
            if (ctx->queue_frames[u] == 0) { rc = -1; continue; }
            const int icl = vcs && vcs[u].n_ref > 0;
            const codec_job_t jb = {u, 0, ctx->queue_frames[u], ctx->queue_codes[u], icl ? vcs[u].ref_codes : NULL,
                                    icl ? vcs[u].n_ref : 0};
            jobs[nj++] = jb;
        }
        const double t_codec = now_ms();
        if (nj > 0 && codec_finish(ctx, dev, nj, jobs, 0, out_audio, out_samples) != 0) rc = -1;
        ctx->perf_codec_ms = now_ms() - t_codec;
    }
    ctx->perf_total_ms = now_ms() - t_start;
    if (qwen_tts_verbose >= 1)
        fprintf(stderr, "Queue: %d utterances on %d slots, %d frames (%lld slot rows), %d refills, occupancy %.3f\n",
                done_n, ns, ctx->queue_frames_launched, ctx->queue_rows_launched, ctx->queue_refills,
                (double)ctx->queue_slot_frames_used / (double)ctx->queue_rows_launched);
out:
    prompts_free(pr, nq);
    free(taken); free(cur); free(first); free(retired); free(hst); free(cbuf); free(jobs);
    if (stream && !finished)   /* a run that failed part-way returns nothing */
        for (int u = 0; u < nq; u++) { free(out_audio[u]); out_audio[u] = NULL; out_samples[u] = 0; }
    sstate_free(&qs);
    free(avail); free(complete); free(ngen);
    sampling_free(sarm);
    instruct_free(iarm);
    free(vcs);
    free(prime_codes);
    return rc;
}

int qwen_tts_generate_queue(qwen_tts_ctx_t *ctx, int nq, const char *const *texts, const char *const *speakers,
                            const char *const *languages, int nb, qwen_tts_queue_next_cb next, void *user,
                            float **out_audio, int *out_samples) {
    return queue_run(ctx, "qwen_tts_generate_queue", nq, texts, speakers, languages, nb, next, user, out_audio,
                     out_samples, NULL, NULL, 0);
}

int qwen_tts_generate_voice_queue(qwen_tts_ctx_t *ctx, int nq, const char *const *texts,
                                  const qwen_tts_voice_t *const *voices, const char *const *languages,
                                  int non_streaming, int nb, qwen_tts_queue_next_cb next, void *user,
                                  float **out_audio, int *out_samples) {
    if (!voices) {
        if (ctx) force_disarm(ctx);
        return -1;
    }
    return queue_run(ctx, "qwen_tts_generate_voice_queue", nq, texts, NULL, languages, nb, next, user, out_audio,
                     out_samples, NULL, voices, non_streaming);
}

/* Reference audio -> what a voice clone takes (create_voice_clone_prompt,
 * qwen3_tts_model.py:356-458): every audio's 12 Hz codes in ONE padded batch
 * (codes [nb][*ld][16], frames[nb]) and each x-vector on its own audio (xv
 * [nb][hidden]); both malloc'd, the caller frees them, also after a failure.
 * -1 with the message for a model without the encoders and for an ICL
 * utterance (x_vector_only NULL or 0 for it) without its ref_text. */
static int ref_audio_encode(qwen_tts_ctx_t *ctx, int nb, const char *const *ref_texts, const float *const *wavs,
                            const int *n_samples, const int *x_vector_only, int **codes, int *ld, int *frames,
                            float **xv) {
    qtts_dev_t *dev = (qtts_dev_t *)ctx->hip;
    *codes = NULL;
    *xv = NULL;
    *ld = 0;
    if ((qtts_dev_enc_available(dev) & 3) != 3) {
        fprintf(stderr, "Error: the model directory has no speaker encoder / 12 Hz encoder weights\n");
        return -1;
    }
    for (int b = 0; b < nb; b++)
        if ((!x_vector_only || !x_vector_only[b]) && (!ref_texts || !ref_texts[b] || !ref_texts[b][0])) {
            fprintf(stderr, "Error: ref_text is required when x_vector_only_mode=False (ICL mode). Bad index=%d\n", b);
            return -1;
        }
    for (int b = 0; b < nb; b++) {
        const int T = (n_samples[b] + 1919) / 1920;
        if (T > *ld) *ld = T;
    }
    *codes = (int *)malloc((size_t)nb * (*ld > 0 ? *ld : 1) * 16 * sizeof(int));
    *xv = (float *)malloc((size_t)nb * ctx->config.talker_hidden * sizeof(float));
    if (!*codes || !*xv) return -1;
    if (qtts_dev_encode_audio(dev, nb, wavs, n_samples, *codes, *ld, frames, NULL) != 0) return -1;
    return qtts_dev_speaker_embed(dev, nb, wavs, n_samples, *xv, NULL);
}

/* ------------------------------------------------------------- voice handles */
static qwen_tts_voice_t *voice_new(qwen_tts_ctx_t *ctx, const char *ref_text, const int *ref_codes, int n_ref,
                                   const float *spk) {
    if (!ctx || !ctx->hip) return NULL;
    const int icl = ref_codes && n_ref > 0, H = ctx->config.talker_hidden;
    if (!icl && !spk) {
        fprintf(stderr, "Error: voice clone needs reference codes or a speaker embedding\n");
        return NULL;
    }
    qwen_tts_voice_t *v = (qwen_tts_voice_t *)calloc(1, sizeof(*v));
    if (!v) return NULL;
    v->ctx = ctx;
    v->hip = ctx->hip;
    if (icl) {
        if ((v->n_ref_ids = ref_text_ids(ctx, ref_text, &v->ref_ids)) < 0) {
            qwen_tts_voice_free(v);
            return NULL;
        }
        v->ref_codes = (int *)malloc((size_t)n_ref * 16 * sizeof(int));
        if (v->ref_codes) memcpy(v->ref_codes, ref_codes, (size_t)n_ref * 16 * sizeof(int));
        v->n_ref = n_ref;
    }
    if (spk) {
        v->spk = (float *)malloc((size_t)H * sizeof(float));
        if (v->spk) memcpy(v->spk, spk, (size_t)H * sizeof(float));
    }
    if ((icl && !v->ref_codes) || (spk && !v->spk)) {
        qwen_tts_voice_free(v);
        return NULL;
    }
    return v;
}

qwen_tts_voice_t *qwen_tts_voice_create(qwen_tts_ctx_t *ctx, const char *ref_text, const int *ref_codes,
                                        int n_ref_frames, const float *spk_embed) {
    return voice_new(ctx, ref_text, ref_codes, n_ref_frames, spk_embed);
}

qwen_tts_voice_t *qwen_tts_voice_create_audio(qwen_tts_ctx_t *ctx, const char *ref_text, const float *ref_wav,
                                              int n_ref_samples, int x_vector_only) {
    if (!ctx || !ctx->hip || !ref_wav || n_ref_samples <= 0) return NULL;
    const char *rt[1] = {ref_text};
    const float *w[1] = {ref_wav};
    const int n[1] = {n_ref_samples}, xo[1] = {x_vector_only};
    int *codes = NULL, ld = 0, fr = 0;
    float *xv = NULL;
    qwen_tts_voice_t *v = NULL;
    if (ref_audio_encode(ctx, 1, rt, w, n, xo, &codes, &ld, &fr, &xv) == 0)
        v = voice_new(ctx, x_vector_only ? NULL : ref_text, x_vector_only ? NULL : codes, x_vector_only ? 0 : fr, xv);
    free(codes);
    free(xv);
    return v;
}

int qwen_tts_voice_info(const qwen_tts_voice_t *v, int *n_ref_frames, int *primed) {
    if (!v) return -1;
    if (n_ref_frames) *n_ref_frames = v->n_ref;
    if (primed) *primed = v->n_ref > 0 && voice_primed(v);
    return 0;
}

void qwen_tts_voice_free(qwen_tts_voice_t *v) {
    if (!v) return;
    qtts_dev_codec_snapshot_free(v->snap);
    free(v->ref_ids); free(v->ref_codes); free(v->spk);
    free(v);
}

qwen_tts_codec_snapshot_t *qwen_tts_codec_mstream_save(qwen_tts_ctx_t *ctx, int stream) {
    if (!ctx || !ctx->hip) return NULL;
    return qtts_dev_codec_mstream_save((qtts_dev_t *)ctx->hip, stream);
}

int qwen_tts_codec_mstream_restore(qwen_tts_ctx_t *ctx, int stream, const qwen_tts_codec_snapshot_t *snap) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_codec_mstream_restore((qtts_dev_t *)ctx->hip, stream, snap);
}

void qwen_tts_codec_snapshot_free(qwen_tts_codec_snapshot_t *snap) { qtts_dev_codec_snapshot_free(snap); }

int qwen_tts_codec_snapshot_pos(const qwen_tts_codec_snapshot_t *snap) { return qtts_dev_codec_snapshot_pos(snap); }

int qwen_tts_queue_codes(qwen_tts_ctx_t *ctx, int i, int *codes, int max_frames) {
    if (!ctx || i < 0 || i >= ctx->queue_n || !ctx->queue_codes || !ctx->queue_codes[i] || max_frames < 0) return -1;
    const int n = ctx->queue_frames[i] < max_frames ? ctx->queue_frames[i] : max_frames;
    if (codes) memcpy(codes, ctx->queue_codes[i], (size_t)n * ctx->config.num_code_groups * sizeof(int));
    return n;
}

static int vclone_run(qwen_tts_ctx_t *ctx, int nb, const char *const *texts, const char *const *ref_texts,
                      const int *const *ref_codes, const int *n_ref_frames, const float *const *spk_embeds,
                      const char *const *languages, int non_streaming, float **out_audio, int *out_samples,
                      const stream_t *stream, double t_start) {
    if (!ctx || nb < 1 || !texts || !out_audio || !out_samples || (stream && !stream->multi && nb != 1)) return -1;
    if (instruct_refuses_clone(ctx, "voice clone")) return -1;
    if (batch_refused(ctx, stream && stream->multi ? "qwen_tts_generate_voice_clone_batch_stream"
                                                   : "qwen_tts_generate_voice_clone_batch", nb))
        return -1;
    for (int b = 0; b < nb; b++) { out_audio[b] = NULL; out_samples[b] = 0; }
    vclone_t *vcs = (vclone_t *)calloc(nb, sizeof(vclone_t));
    int rc = vcs ? 0 : -1;
    for (int b = 0; b < nb && rc == 0; b++) {
        vclone_t *vc = &vcs[b];
        const int *codes = ref_codes ? ref_codes[b] : NULL;
        const int nref = n_ref_frames ? n_ref_frames[b] : 0;
        vc->spk = spk_embeds ? spk_embeds[b] : NULL;
        vc->non_streaming = non_streaming;
        if (!(codes && nref > 0)) {
            if (!vc->spk) {
                fprintf(stderr, "Error: voice clone needs reference codes or a speaker embedding\n");
                rc = -1;
            }
            continue;
        }
        int *rid = NULL;
        vc->n_ref_ids = ref_text_ids(ctx, ref_texts ? ref_texts[b] : NULL, &rid);
        vc->ref_ids = rid;
        if (vc->n_ref_ids < 0) rc = -1;
        vc->ref_codes = codes;
        vc->n_ref = nref;
    }
    if (rc == 0)
        rc = run_batch(ctx, nb, texts, NULL, languages, out_audio, out_samples, t_start > 0 ? t_start : now_ms(), stream,
                       vcs);
    else force_disarm(ctx);   /* (the call consumes an arming also when it fails before the run) */
    if (vcs)
        for (int b = 0; b < nb; b++) free((void *)vcs[b].ref_ids);
    free(vcs);
    return rc;
}

int qwen_tts_generate_voice_clone_batch(qwen_tts_ctx_t *ctx, int nb, const char *const *texts,
                                        const char *const *ref_texts, const int *const *ref_codes,
                                        const int *n_ref_frames, const float *const *spk_embeds,
                                        const char *const *languages, int non_streaming, float **out_audio,
                                        int *out_samples) {
    return vclone_run(ctx, nb, texts, ref_texts, ref_codes, n_ref_frames, spk_embeds, languages, non_streaming,
                      out_audio, out_samples, NULL, 0);
}

static int vclone_batch_stream(qwen_tts_ctx_t *ctx, int nb, const char *const *texts, const char *const *ref_texts,
                               const int *const *ref_codes, const int *n_ref_frames, const float *const *spk_embeds,
                               const char *const *languages, int non_streaming, int chunk_frames,
                               qwen_tts_batch_audio_cb cb, void *userdata, float **out_audio, int *out_samples,
                               double t_start) {
    stream_t st = {NULL, userdata, chunk_frames > 0 ? chunk_frames : 1, 1, cb};
    if (ctx) ctx->perf_first_packet_ms = 0;
    const int rc = vclone_run(ctx, nb, texts, ref_texts, ref_codes, n_ref_frames, spk_embeds, languages, non_streaming,
                              out_audio, out_samples, &st, t_start);
    if (rc == 0) log_totals(ctx, 1, 1, nb, out_samples);
    return rc;
}

int qwen_tts_generate_voice_clone_batch_stream(qwen_tts_ctx_t *ctx, int nb, const char *const *texts,
                                               const char *const *ref_texts, const int *const *ref_codes,
                                               const int *n_ref_frames, const float *const *spk_embeds,
                                               const char *const *languages, int non_streaming, int chunk_frames,
                                               qwen_tts_batch_audio_cb cb, void *userdata, float **out_audio,
                                               int *out_samples) {
    return vclone_batch_stream(ctx, nb, texts, ref_texts, ref_codes, n_ref_frames, spk_embeds, languages,
                               non_streaming, chunk_frames, cb, userdata, out_audio, out_samples, now_ms());
}

/* one utterance through vclone_run (st NULL: not streamed) */
static float *vclone_one(qwen_tts_ctx_t *ctx, const char *text, const char *ref_text, const int *ref_codes,
                         int n_ref_frames, const float *spk_embed, const char *language, int non_streaming,
                         const stream_t *st, int *out_samples) {
    if (!ctx || !out_samples) return NULL;
    *out_samples = 0;
    float *audio = NULL;
    int n = 0;
    const char *texts[1] = {text}, *rt[1] = {ref_text}, *lang[1] = {language};
    const int *rc1[1] = {ref_codes};
    const int nr1[1] = {n_ref_frames};
    const float *sv1[1] = {spk_embed};
    if (st) ctx->perf_first_packet_ms = 0;
    const int rc = vclone_run(ctx, 1, texts, rt, rc1, nr1, sv1, lang, non_streaming, &audio, &n, st, 0);
    return one_result(rc, audio, n, out_samples);
}

float *qwen_tts_generate_voice_clone_stream(qwen_tts_ctx_t *ctx, const char *text, const char *ref_text,
                                            const int *ref_codes, int n_ref_frames, const float *spk_embed,
                                            const char *language, int non_streaming, int chunk_frames,
                                            qwen_tts_audio_cb cb, void *userdata, int *out_samples) {
    const stream_t st = {cb, userdata, chunk_frames > 0 ? chunk_frames : 1};
    return vclone_one(ctx, text, ref_text, ref_codes, n_ref_frames, spk_embed, language, non_streaming, &st,
                      out_samples);
}

float *qwen_tts_generate_voice_clone(qwen_tts_ctx_t *ctx, const char *text, const char *ref_text,
                                     const int *ref_codes, int n_ref_frames, const float *spk_embed,
                                     const char *language, int non_streaming, int *out_samples) {
    return vclone_one(ctx, text, ref_text, ref_codes, n_ref_frames, spk_embed, language, non_streaming, NULL,
                      out_samples);
}

/* ------------------------------------------- voice clone from reference audio (N3) */
float *qwen_tts_speaker_embedding(qwen_tts_ctx_t *ctx, const float *wav, int n_samples, int *out_dim) {
    if (out_dim) *out_dim = 0;
    if (!ctx || !ctx->hip || !wav || n_samples <= 0) return NULL;
    const int dim = ctx->config.talker_hidden;
    float *out = (float *)malloc((size_t)dim * sizeof(float));
    if (!out) return NULL;
    const float *w[1] = {wav};
    const int n[1] = {n_samples};
    if (qtts_dev_speaker_embed((qtts_dev_t *)ctx->hip, 1, w, n, out, NULL) != 0) {
        free(out);
        return NULL;
    }
    if (out_dim) *out_dim = dim;
    return out;
}

int *qwen_tts_encode_audio(qwen_tts_ctx_t *ctx, const float *wav, int n_samples, int *out_frames) {
    if (out_frames) *out_frames = 0;
    if (!ctx || !ctx->hip || !wav || n_samples <= 0) return NULL;
    const int T = (n_samples + 1919) / 1920;
    int *codes = (int *)malloc((size_t)T * 16 * sizeof(int));
    if (!codes) return NULL;
    const float *w[1] = {wav};
    const int n[1] = {n_samples};
    int fr = 0;
    if (qtts_dev_encode_audio((qtts_dev_t *)ctx->hip, 1, w, n, codes, T, &fr, NULL) != 0) {
        free(codes);
        return NULL;
    }
    if (out_frames) *out_frames = fr;
    return codes;
}

/* generate_voice_clone on reference audio: the audio is encoded
 * (ref_audio_encode), then the codes / x-vector voice clone above.
 * x_vector_only[b] (NULL: all 0) drops the codes of slot b (ref_code=None,
 * qwen3_tts_model.py:451). */
typedef struct {                 /* the streamed form's extra arguments */
    int chunk_frames;
    qwen_tts_batch_audio_cb cb;
    void *userdata;
} vc_bstream_t;

static int vclone_audio_run(qwen_tts_ctx_t *ctx, int nb, const char *const *texts, const char *const *ref_texts,
                            const float *const *ref_wavs, const int *n_ref_samples, const char *const *languages,
                            const int *x_vector_only, int non_streaming, float **out_audio, int *out_samples,
                            const vc_bstream_t *bs) {
    if (!ctx || !ctx->hip || nb < 1 || nb > 16 || !texts || !ref_wavs || !n_ref_samples || !out_audio ||
        !out_samples) {
        fprintf(stderr, "Error: voice clone from audio needs 1..16 utterances with reference audio\n");
        if (ctx) force_disarm(ctx);
        return -1;
    }
    if (instruct_refuses_clone(ctx, "voice clone from audio")) return -1;
    for (int b = 0; b < nb; b++) { out_audio[b] = NULL; out_samples[b] = 0; }
    const double t0 = now_ms();
    const int H = ctx->config.talker_hidden;
    int *codes = NULL, maxT = 0, frames[16], rc = -1;
    float *xv = NULL;
    if (ref_audio_encode(ctx, nb, ref_texts, ref_wavs, n_ref_samples, x_vector_only, &codes, &maxT, frames, &xv) == 0) {
        const int *rc_p[16];
        int nr[16];
        const float *sv[16];
        for (int b = 0; b < nb; b++) {
            const int xo = x_vector_only && x_vector_only[b];
            rc_p[b] = xo ? NULL : codes + (size_t)b * maxT * 16;
            nr[b] = xo ? 0 : frames[b];
            sv[b] = xv + (size_t)b * H;
        }
        if (qwen_tts_verbose >= 1) fprintf(stderr, "Reference audio encoded in %.1f ms\n", now_ms() - t0);
        const char *const *rt = ref_texts;
        const char *none[16] = {NULL};
        if (!rt) rt = none;
        /* (streamed: the first packet counts from this call's entry, the encoders included) */
        if (bs)
            rc = vclone_batch_stream(ctx, nb, texts, rt, rc_p, nr, sv, languages, non_streaming, bs->chunk_frames,
                                     bs->cb, bs->userdata, out_audio, out_samples, t0);
        else
            rc = qwen_tts_generate_voice_clone_batch(ctx, nb, texts, rt, rc_p, nr, sv, languages, non_streaming,
                                                     out_audio, out_samples);
    } else {
        force_disarm(ctx);   /* (the call consumes an arming also when it fails before the run) */
    }
    free(codes);
    free(xv);
    return rc;
}

int qwen_tts_generate_voice_clone_audio_batch(qwen_tts_ctx_t *ctx, int nb, const char *const *texts,
                                              const char *const *ref_texts, const float *const *ref_wavs,
                                              const int *n_ref_samples, const char *const *languages,
                                              const int *x_vector_only, int non_streaming, float **out_audio,
                                              int *out_samples) {
    return vclone_audio_run(ctx, nb, texts, ref_texts, ref_wavs, n_ref_samples, languages, x_vector_only,
                            non_streaming, out_audio, out_samples, NULL);
}

int qwen_tts_generate_voice_clone_audio_batch_stream(qwen_tts_ctx_t *ctx, int nb, const char *const *texts,
                                                     const char *const *ref_texts, const float *const *ref_wavs,
                                                     const int *n_ref_samples, const char *const *languages,
                                                     const int *x_vector_only, int non_streaming, int chunk_frames,
                                                     qwen_tts_batch_audio_cb cb, void *userdata, float **out_audio,
                                                     int *out_samples) {
    const vc_bstream_t bs = {chunk_frames, cb, userdata};
    return vclone_audio_run(ctx, nb, texts, ref_texts, ref_wavs, n_ref_samples, languages, x_vector_only,
                            non_streaming, out_audio, out_samples, &bs);
}

/* streaming form of qwen_tts_generate_voice_clone_audio: the reference audio
 * is encoded first, then qwen_tts_generate_voice_clone_stream; the first
 * packet time (ctx->perf_first_packet_ms) counts from this call's entry */
float *qwen_tts_generate_voice_clone_audio_stream(qwen_tts_ctx_t *ctx, const char *text, const char *ref_text,
                                                  const float *ref_wav, int n_ref_samples, const char *language,
                                                  int x_vector_only, int non_streaming, int chunk_frames,
                                                  qwen_tts_audio_cb cb, void *userdata, int *out_samples) {
    if (!out_samples) return NULL;
    *out_samples = 0;
    if (!ctx || !ctx->hip || !ref_wav || n_ref_samples <= 0) {
        if (ctx) force_disarm(ctx);
        return NULL;
    }
    if (instruct_refuses_clone(ctx, "voice clone from audio")) return NULL;
    const double t0 = now_ms();
    const char *rt[1] = {ref_text};
    const float *w[1] = {ref_wav};
    const int n[1] = {n_ref_samples}, xo[1] = {x_vector_only};
    int *codes = NULL, ld = 0, fr = 0;
    float *xv = NULL, *audio = NULL;
    if (ref_audio_encode(ctx, 1, rt, w, n, xo, &codes, &ld, &fr, &xv) == 0) {
        const double enc_ms = now_ms() - t0;
        audio = qwen_tts_generate_voice_clone_stream(ctx, text, x_vector_only ? NULL : ref_text,
                                                     x_vector_only ? NULL : codes, x_vector_only ? 0 : fr, xv,
                                                     language, non_streaming, chunk_frames, cb, userdata, out_samples);
        if (audio && ctx->perf_first_packet_ms > 0) ctx->perf_first_packet_ms += enc_ms;
    } else {
        force_disarm(ctx);
    }
    free(codes);
    free(xv);
    return audio;
}

float *qwen_tts_generate_voice_clone_audio(qwen_tts_ctx_t *ctx, const char *text, const char *ref_text,
                                           const float *ref_wav, int n_ref_samples, const char *language,
                                           int x_vector_only, int non_streaming, int *out_samples) {
    if (!out_samples) return NULL;
    *out_samples = 0;
    float *audio = NULL;
    int n = 0;
    const char *texts[1] = {text}, *rt[1] = {ref_text}, *lang[1] = {language};
    const float *w[1] = {ref_wav};
    const int nn[1] = {n_ref_samples}, xo[1] = {x_vector_only};
    const int rc = qwen_tts_generate_voice_clone_audio_batch(ctx, 1, texts, rt, w, nn, lang, xo, non_streaming, &audio, &n);
    return one_result(rc, audio, n, out_samples);
}

float *qwen_tts_generate_stream(qwen_tts_ctx_t *ctx, const char *text, const char *speaker, const char *language,
                                int chunk_frames, qwen_tts_audio_cb cb, void *userdata, int *out_samples) {
    if (!ctx || !out_samples) return NULL;
    *out_samples = 0;
    double t_start = now_ms();
    stream_t st = {cb, userdata, chunk_frames > 0 ? chunk_frames : 1};
    float *audio = NULL;
    int n = 0;
    const char *texts[1] = {text}, *spk[1] = {speaker}, *lang[1] = {language};
    ctx->perf_first_packet_ms = 0;
    const int rc = run_batch(ctx, 1, texts, spk, lang, &audio, &n, t_start, &st, NULL);
    audio = one_result(rc, audio, n, out_samples);
    if (audio) log_totals(ctx, 1, 0, 1, &n);
    return audio;
}

int qwen_tts_generate_batch_stream(qwen_tts_ctx_t *ctx, int nb, const char *const *texts,
                                   const char *const *speakers, const char *const *languages, int chunk_frames,
                                   qwen_tts_batch_audio_cb cb, void *userdata, float **out_audio, int *out_samples) {
    if (!ctx || nb < 1 || !texts || !out_audio || !out_samples) return -1;
    if (batch_refused(ctx, "qwen_tts_generate_batch_stream", nb)) return -1;
    const double t_start = now_ms();
    stream_t st = {NULL, userdata, chunk_frames > 0 ? chunk_frames : 1, 1, cb};
    ctx->perf_first_packet_ms = 0;
    const int rc = run_batch(ctx, nb, texts, speakers, languages, out_audio, out_samples, t_start, &st, NULL);
    if (rc == 0) log_totals(ctx, 1, 1, nb, out_samples);
    return rc;
}

/* ------------------------------------------------- incremental text input */
/* The two device entries of a fed run are weak here: a build of this file
 * against a device layer without them (the host-trace fakes of the other
 * calls) links, and the fed calls refuse. */
extern int qtts_dev_text_open(qtts_dev_t *dev, int b) __attribute__((weak));
extern int qtts_dev_text_append(qtts_dev_t *dev, int b, const int *ids, int n, int close) __attribute__((weak));

/* One fed call's text state.  Before the device run has begun (dev NULL) the
 * ids are kept here; from then on a push is one qtts_dev_text_append.  With
 * content ids c[0..m) trailing row r is proj(c[r + 1]), row m - 1 tts_eos, and
 * the frame that draws frame r needs row r: utterance u is starved when its
 * text is open and frames[u] >= rows[u], all of it host arithmetic. */
#define FEED_TOKEN_ASSISTANT 77091   /* "assistant" and "\n" of "<|im_start|>assistant\n" */
#define FEED_TOKEN_NEWLINE 198
struct qwen_tts_feed {
    const qwen_tts_ctx_t *ctx;
    qtts_dev_t *dev;
    int nb, in_cb, failed;
    int **ids;                   /* [nb] ids pushed before the device run began */
    int *cap;
    int *taken, *closed, *rows;  /* ids taken; the text is over; trailing rows published (tts_eos included) */
    int *frames, *stopped;       /* frames launched for it; it drew EOS or reached the limit */
    int *touched;                /* pushed or closed during the current callback */
};

static void feed_free(qwen_tts_feed_t *f) {
    for (int u = 0; f->ids && u < f->nb; u++) free(f->ids[u]);
    free(f->ids); free(f->cap); free(f->taken); free(f->closed); free(f->rows); free(f->frames); free(f->stopped);
    free(f->touched);
    memset(f, 0, sizeof *f);
}

static int feed_init(qwen_tts_feed_t *f, const qwen_tts_ctx_t *ctx, int nb) {
    memset(f, 0, sizeof *f);
    f->ctx = ctx;
    f->nb = nb;
    f->ids = (int **)calloc(nb, sizeof(int *));
    f->cap = (int *)calloc(nb, sizeof(int)); f->taken = (int *)calloc(nb, sizeof(int));
    f->closed = (int *)calloc(nb, sizeof(int)); f->rows = (int *)calloc(nb, sizeof(int));
    f->frames = (int *)calloc(nb, sizeof(int)); f->stopped = (int *)calloc(nb, sizeof(int));
    f->touched = (int *)calloc(nb, sizeof(int));
    return f->ids && f->cap && f->taken && f->closed && f->rows && f->frames && f->stopped && f->touched ? 0 : -1;
}

static int feed_starved(const qwen_tts_feed_t *f, int u) {
    return !f->stopped[u] && !f->closed[u] && (f->taken[u] < 1 || f->frames[u] >= f->rows[u]);
}

/* the checks every push and close starts with: 1 go on, 0 nothing to do, -1 refused */
static int feed_enter(qwen_tts_feed_t *f, int u, const char *who) {
    if (!f || !f->in_cb) {
        fprintf(stderr, "Error: %s: valid only inside the feed callback\n", who);
        return -1;
    }
    if (u < 0 || u >= f->nb) {
        fprintf(stderr, "Error: %s: utterance %d of %d\n", who, u, f->nb);
        return -1;
    }
    if (f->stopped[u]) return 0;
    if (f->closed[u]) {
        fprintf(stderr, "Error: %s: utterance %d is closed\n", who, u);
        return -1;
    }
    return 1;
}

static int feed_put(qwen_tts_feed_t *f, int u, const int *ids, int n, int close) {
    if (f->dev) {
        /* (the first id is in the prefill; every later one is a trailing row) */
        if (qtts_dev_text_append(f->dev, u, ids, n, close) != 0) { f->failed = 1; return -1; }
        f->rows[u] += n + close;
    } else {
        if (f->taken[u] + n > f->cap[u]) {
            const int cap = (f->taken[u] + n) * 2 + 16;
            int *p = (int *)realloc(f->ids[u], (size_t)cap * sizeof(int));
            if (!p) { f->failed = 1; return -1; }
            f->ids[u] = p;
            f->cap[u] = cap;
        }
        if (n) memcpy(f->ids[u] + f->taken[u], ids, (size_t)n * sizeof(int));
    }
    f->taken[u] += n;
    if (close) f->closed[u] = 1;
    f->touched[u] = 1;
    return 0;
}

int qwen_tts_feed_ids(qwen_tts_feed_t *feed, int utterance, const int *ids, int n) {
    const int go = feed_enter(feed, utterance, "qwen_tts_feed_ids");
    if (go <= 0) return go;
    if (!ids || n < 1) {
        fprintf(stderr, "Error: qwen_tts_feed_ids: %d ids\n", n);
        return -1;
    }
    if (!ids_in_range(feed->ctx, ids, n)) return -1;
    return feed_put(feed, utterance, ids, n, 0);
}

int qwen_tts_feed_close(qwen_tts_feed_t *feed, int utterance) {
    const int go = feed_enter(feed, utterance, "qwen_tts_feed_close");
    if (go <= 0) return go;
    return feed_put(feed, utterance, NULL, 0, 1);
}

int qwen_tts_feed_state(const qwen_tts_feed_t *feed, int utterance, int *ids_taken, int *frames_done, int *starved) {
    if (!feed || utterance < 0 || utterance >= feed->nb) return -1;
    if (ids_taken) *ids_taken = feed->taken[utterance];
    if (frames_done) *frames_done = feed->frames[utterance];
    if (starved) *starved = feed_starved(feed, utterance);
    return 0;
}

/* One callback.  wait: afterwards some utterance that was starved on entry
 * must have been pushed to or closed, or the loop would spin. */
static int feed_call(qwen_tts_feed_t *f, qwen_tts_text_feed_cb cb, void *user, int wait) {
    int was[QWEN_TTS_MAX_BATCH], progress = 0;
    for (int u = 0; u < f->nb; u++) {
        was[u] = feed_starved(f, u);
        f->touched[u] = 0;
    }
    f->in_cb = 1;
    const int rc = cb(f, wait, user);
    f->in_cb = 0;
    if (rc < 0) {
        fprintf(stderr, "Error: the feed callback aborted the call (%d)\n", rc);
        return -1;
    }
    if (f->failed) return -1;
    for (int u = 0; u < f->nb; u++) progress |= was[u] && f->touched[u];
    if (wait && !progress) {
        fprintf(stderr, "Error: feed made no progress (a wait = 1 callback pushed nothing for a starved utterance)\n");
        return -1;
    }
    return 0;
}

static int run_fed(qwen_tts_ctx_t *ctx, int nb, const char *const *speakers, const char *const *languages,
                   const stream_t *stream, qwen_tts_text_feed_cb feed_cb, void *feed_user, float **audio,
                   int *samples, double t_start) {
    qtts_dev_t *dev = (qtts_dev_t *)ctx->hip;
    const int G = ctx->config.num_code_groups;
    int rc = -1;
    sampling_arm_t *sarm = sampling_take(ctx);
    instruct_arm_t *iarm = instruct_take(ctx);
    prompt_t *pr = NULL;
    int *stopped = NULL, *ngen = NULL, *sstep = NULL, *retired = NULL;
    sstate_t ss;
    qwen_tts_feed_t fd;
    memset(&ss, 0, sizeof ss);
    memset(&fd, 0, sizeof fd);
    if (sampling_refused("generate_fed", sarm, NULL, nb) || instruct_refused("generate_fed", iarm, nb, 0)) goto out;
    if (!qtts_dev_text_open || !qtts_dev_text_append) {
        fprintf(stderr, "Error: generate_fed: this build's device layer has no incremental text input\n");
        goto out;
    }
    const int fixed = ctx->fixed_codec_tokens > 0 ? ctx->fixed_codec_tokens : 0;
    const int max_tokens = fixed > 0 ? fixed : ctx->max_new_tokens;
    if (max_tokens < 1) goto out;
    if (feed_init(&fd, ctx, nb) != 0) goto out;
    /* start: every utterance's first content id, before the device is touched */
    for (;;) {
        int missing = 0;
        for (int u = 0; u < nb; u++) {
            if (fd.taken[u] > 0) continue;
            if (fd.closed[u]) {
                fprintf(stderr, "Error: generate_fed: utterance %d was closed without an id\n", u);
                goto out;
            }
            missing = 1;
        }
        if (!missing) break;
        if (feed_call(&fd, feed_cb, feed_user, 1) != 0) goto out;
    }
    if (!(pr = (prompt_t *)calloc(nb, sizeof(prompt_t)))) goto out;
    int max_p = 0;
    for (int b = 0; b < nb; b++) {
        /* build_prompt's layout of a template whose one content id is this id:
         * role ids, id, and the five closing ids it never reads */
        const int tpl[9] = {QWEN_TTS_TOKEN_IM_START, FEED_TOKEN_ASSISTANT, FEED_TOKEN_NEWLINE, fd.ids[b][0], 0, 0, 0, 0, 0};
        int spk, lang;
        lookup(ctx, speakers ? speakers[b] : NULL, languages ? languages[b] : NULL, &spk, &lang);
        if (build_prompt(ctx, tpl, 9, spk, lang, iarm ? iarm->ids[b] : NULL, iarm ? iarm->n_ids[b] : 0, b, &pr[b]) != 0)
            goto out;
        if (pr[b].p_len > max_p) max_p = pr[b].p_len;
    }
    qtts_gen_params_t gp;
    params_of(ctx, &gp);
    if (qtts_dev_begin(dev, nb, max_tokens, max_p, &gp) != 0) goto out;
    if (sarm)
        for (int b = 0; b < nb; b++)
            if (sampling_apply(dev, sarm, b, b) != 0) goto out;
    for (int b = 0; b < nb; b++)
        if (qtts_dev_prompt(dev, b, pr[b].text, pr[b].n_text, pr[b].plan, pr[b].nplan, pr[b].p_len, pr[b].n_trailing,
                            pr[b].pad_row) != 0 ||
            qtts_dev_text_open(dev, b) != 0)
            goto out;
    /* what came with the first ids goes to the device; later pushes go there directly */
    for (int b = 0; b < nb; b++) {
        const int n = fd.taken[b] - 1;
        if ((n > 0 || fd.closed[b]) && qtts_dev_text_append(dev, b, fd.ids[b] + 1, n, fd.closed[b]) != 0) goto out;
        fd.rows[b] = n + fd.closed[b];
    }
    fd.dev = dev;
    if (qtts_dev_codec_mstream_begin(dev, nb, max_tokens, 0) != 0) goto out;
    double t_prefill = now_ms();
    if (qtts_dev_prefill(dev) != 0) goto out;
    ctx->perf_prefill_ms = now_ms() - t_prefill;
    stopped = (int *)calloc(nb, sizeof(int)); ngen = (int *)calloc(nb, sizeof(int));
    sstep = (int *)calloc(nb, sizeof(int)); retired = (int *)calloc(nb, sizeof(int));
    if (!stopped || !ngen || !sstep || !retired) goto out;
    if (sstate_init(&ss, stream, nb, max_tokens, t_start, 0) != 0) goto out;
    const double t_gen = now_ms();
    int launched = 0, since_poll = 0;
    for (;;) {
        int live = 0, starved = 0, furthest = 0;
        for (int b = 0; b < nb; b++) {
            if (!fd.stopped[b] && fd.frames[b] >= max_tokens) {   /* the frame limit: stopped from the next launch on */
                if (!retired[b] && qtts_dev_retire(dev, b) != 0) goto out;
                retired[b] = fd.stopped[b] = 1;
            }
            live += !fd.stopped[b];
        }
        if (!live) break;
        if (feed_call(&fd, feed_cb, feed_user, 0) != 0) goto out;
        for (int b = 0; b < nb; b++) starved += feed_starved(&fd, b);
        /* frame 0 is the lock-step head on the prefill's hidden states: every slot needs its row */
        const int hold_all = launched == 0 ? starved > 0 : starved == live;
        int polled = 0;
        if (hold_all) {
            /* nothing can advance: what is decoded goes out first, then the feed may block */
            if (since_poll) polled = 1;
        } else {
            if (qtts_dev_frame(dev, launched) != 0) goto out;
            for (int b = 0; b < nb; b++)
                if (!fd.stopped[b] && !feed_starved(&fd, b)) fd.frames[b]++;
            launched++;
            since_poll++;
            if (launched == 1) {
                qtts_dev_poll(dev, NULL, NULL, NULL);
                ctx->perf_first_frame_ms = now_ms() - t_start;
            }
            if (ctx->progress_cb) ctx->progress_cb(launched, max_tokens, ctx->progress_cb_userdata);
            /* delivery: frame 0, then whenever a slot has chunk_frames new frames, and a slot's tail
             * as soon as it reaches the limit (EOS mode also looks for stops every 8 launches) */
            int tail = 0;
            for (int b = 0; b < nb; b++) {
                if (fd.frames[b] - ss.done[b] > furthest) furthest = fd.frames[b] - ss.done[b];
                tail |= !fd.stopped[b] && fd.frames[b] >= max_tokens;
            }
            polled = launched == 1 || furthest >= stream->chunk || tail || (!fixed && since_poll >= 8);
        }
        if (polled) {
            if (qtts_dev_poll(dev, stopped, ngen, sstep) != 0) goto out;
            since_poll = 0;
            for (int b = 0; b < nb; b++) {
                /* the host's mirror of the gate against the device's counters
                 * (an EOS: the frame that drew it stored nothing, and the host
                 * went on counting until this poll) */
                const int eos = stopped[b] && !retired[b];
                if (eos ? ngen[b] > fd.frames[b] : ngen[b] != fd.frames[b]) {
                    fprintf(stderr, "Error: generate_fed: utterance %d has %d frames on the device, %d by the host's "
                                    "count of its text rows\n", b, ngen[b], fd.frames[b]);
                    goto out;
                }
                if (eos) {
                    fd.frames[b] = ngen[b];
                    fd.stopped[b] = 1;
                }
            }
            if (batch_flush(ctx, dev, &ss, ngen, 1) != 0) goto out;
        }
        if (hold_all) {
            live = 0;
            for (int b = 0; b < nb; b++) live += !fd.stopped[b];   /* (the poll may have seen the last EOS) */
            if (live && feed_call(&fd, feed_cb, feed_user, 1) != 0) goto out;
        }
    }
    if (qtts_dev_poll(dev, stopped, ngen, sstep) != 0) goto out;
    if (batch_flush(ctx, dev, &ss, ngen, 1) != 0) goto out;
    ctx->perf_talker_ms = now_ms() - t_gen - ss.t_stream;
    ctx->perf_codec_ms = ss.t_stream;
    ctx->perf_codec_tokens = ngen[0];
    ctx->last_stop_reason = stopped[0] && !retired[0] ? 1 : 2;
    ctx->last_stop_step = stopped[0] && !retired[0] ? sstep[0] : max_tokens;
    free(ctx->last_codes);
    ctx->last_codes = (int *)malloc((size_t)(ngen[0] > 0 ? ngen[0] : 1) * G * sizeof(int));
    ctx->last_frames = ngen[0] > 0 && ctx->last_codes ? qtts_dev_get_codes(dev, 0, ctx->last_codes, ngen[0]) : 0;
    if (ctx->last_frames < 0) ctx->last_frames = 0;
    rc = 0;
    for (int b = 0; b < nb; b++) {
        audio[b] = ss.buf[b];
        ss.buf[b] = NULL;
        samples[b] = ss.done[b] * 1920;
        if (ss.done[b] <= 0) rc = -1;
    }
    if (rc != 0)   /* a failed call returns nothing */
        for (int b = 0; b < nb; b++) { free(audio[b]); audio[b] = NULL; samples[b] = 0; }
    ctx->perf_total_ms = now_ms() - t_start;
out:
    sampling_free(sarm);
    instruct_free(iarm);
    free(stopped); free(ngen); free(sstep); free(retired);
    sstate_free(&ss);
    prompts_free(pr, nb);
    feed_free(&fd);
    return rc;
}

int qwen_tts_generate_fed_batch_stream(qwen_tts_ctx_t *ctx, int nb, const char *const *speakers,
                                       const char *const *languages, int chunk_frames, qwen_tts_text_feed_cb feed_cb,
                                       void *feed_userdata, qwen_tts_batch_audio_cb audio_cb, void *audio_userdata,
                                       float **out_audio, int *out_samples) {
    if (!ctx || !out_audio || !out_samples) return -1;
    for (int i = 0; i < nb; i++) { out_audio[i] = NULL; out_samples[i] = 0; }   /* a failed call returns nothing */
    if (nb < 1 || !feed_cb) {
        fprintf(stderr, "Error: qwen_tts_generate_fed_batch_stream: %s\n", nb < 1 ? "no utterances" : "no feed callback");
        force_disarm(ctx);
        return -1;
    }
    if (batch_refused(ctx, "qwen_tts_generate_fed_batch_stream", nb)) return -1;
    if (ctx->force) {
        fprintf(stderr, "Error: qwen_tts_generate_fed_batch_stream: forced codes / taps are armed (not supported "
                        "with incremental text; disarmed)\n");
        force_disarm(ctx);
        return -1;
    }
    const double t_start = now_ms();
    stream_t st = {NULL, audio_userdata, chunk_frames > 0 ? chunk_frames : 1, 1, audio_cb};
    ctx->perf_first_packet_ms = 0;
    const int rc = run_fed(ctx, nb, speakers, languages, &st, feed_cb, feed_userdata, out_audio, out_samples, t_start);
    if (rc == 0) log_totals(ctx, 1, 1, nb, out_samples);
    return rc;
}

/* the single call is the nb = 1 case: the batch callback hands on to the plain one */
typedef struct { qwen_tts_audio_cb cb; void *user; } fed_one_t;
static void fed_one_cb(int utterance, const float *pcm, int n_samples, void *userdata) {
    const fed_one_t *o = (const fed_one_t *)userdata;
    (void)utterance;
    if (o->cb) o->cb(pcm, n_samples, o->user);
}

float *qwen_tts_generate_fed_stream(qwen_tts_ctx_t *ctx, const char *speaker, const char *language, int chunk_frames,
                                    qwen_tts_text_feed_cb feed_cb, void *feed_userdata, qwen_tts_audio_cb audio_cb,
                                    void *audio_userdata, int *out_samples) {
    if (!ctx || !out_samples) return NULL;
    *out_samples = 0;
    fed_one_t one = {audio_cb, audio_userdata};
    float *audio = NULL;
    int n = 0;
    const char *spk[1] = {speaker}, *lang[1] = {language};
    const int rc = qwen_tts_generate_fed_batch_stream(ctx, 1, spk, lang, chunk_frames, feed_cb, feed_userdata,
                                                      fed_one_cb, &one, &audio, &n);
    return one_result(rc, audio, n, out_samples);
}

int qwen_tts_codec_mstream_begin(qwen_tts_ctx_t *ctx, int n_streams, int max_frames) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_codec_mstream_begin((qtts_dev_t *)ctx->hip, n_streams, max_frames, 0);
}

int qwen_tts_codec_mstream_push(qwen_tts_ctx_t *ctx, int n, const int *streams, const int *codes, int time_steps,
                                float *const *out) {
    if (!ctx || !ctx->hip || !streams || !codes || !out) return -1;
    return qtts_dev_codec_mstream_push_host((qtts_dev_t *)ctx->hip, n, streams, codes, time_steps, out);
}

int qwen_tts_codec_mstream_push_any(qwen_tts_ctx_t *ctx, int n, const int *streams, const int *codes, int time_steps,
                                    float *const *out) {
    if (!ctx || !ctx->hip || !streams || !codes || !out) return -1;
    return qtts_dev_codec_mstream_push_host_any((qtts_dev_t *)ctx->hip, n, streams, codes, time_steps, out);
}

int qwen_tts_codec_mstream_push_ragged(qwen_tts_ctx_t *ctx, int n, const int *streams, const int *codes,
                                       const int *counts, int ld_frames, float *const *out) {
    if (!ctx || !ctx->hip || !streams || !codes || !out) return -1;
    /* (a NULL counts is the device layer's refusal, with its message) */
    return qtts_dev_codec_mstream_push_host_ragged((qtts_dev_t *)ctx->hip, n, streams, codes, counts, ld_frames, out);
}

int qwen_tts_codec_mstream_reset(qwen_tts_ctx_t *ctx, int stream) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_codec_mstream_reset((qtts_dev_t *)ctx->hip, stream);
}

static int queue_stream_run(qwen_tts_ctx_t *ctx, const char *who, int nq, const char *const *texts,
                            const char *const *speakers, const qwen_tts_voice_t *const *voices,
                            const char *const *languages, int non_streaming, int nb, qwen_tts_queue_next_cb next,
                            void *userdata, int chunk_frames, qwen_tts_batch_audio_cb cb, void *cb_userdata,
                            float **out_audio, int *out_samples) {
    /* (the slot limit is named whatever else is wrong with the call: before the device is looked at) */
    if (ctx && !ctx->force && batch_refused(ctx, who, nb)) return -1;
    stream_t st = {NULL, cb_userdata, chunk_frames > 0 ? chunk_frames : 1, 1, cb};
    if (ctx) ctx->perf_first_packet_ms = 0;
    const int rc = queue_run(ctx, who, nq, texts, speakers, languages, nb, next, userdata, out_audio, out_samples, &st,
                             voices, non_streaming);
    if (rc == 0) log_totals(ctx, 1, 1, nq, out_samples);
    return rc;
}

int qwen_tts_generate_queue_stream(qwen_tts_ctx_t *ctx, int nq, const char *const *texts, const char *const *speakers,
                                   const char *const *languages, int nb, qwen_tts_queue_next_cb next, void *userdata,
                                   int chunk_frames, qwen_tts_batch_audio_cb cb, void *cb_userdata, float **out_audio,
                                   int *out_samples) {
    return queue_stream_run(ctx, "qwen_tts_generate_queue_stream", nq, texts, speakers, NULL, languages, 0, nb, next,
                            userdata, chunk_frames, cb, cb_userdata, out_audio, out_samples);
}

int qwen_tts_generate_voice_queue_stream(qwen_tts_ctx_t *ctx, int nq, const char *const *texts,
                                         const qwen_tts_voice_t *const *voices, const char *const *languages,
                                         int non_streaming, int nb, qwen_tts_queue_next_cb next, void *userdata,
                                         int chunk_frames, qwen_tts_batch_audio_cb cb, void *cb_userdata,
                                         float **out_audio, int *out_samples) {
    if (!voices) {
        if (ctx) force_disarm(ctx);
        return -1;
    }
    return queue_stream_run(ctx, "qwen_tts_generate_voice_queue_stream", nq, texts, NULL, voices, languages,
                            non_streaming, nb, next, userdata, chunk_frames, cb, cb_userdata, out_audio, out_samples);
}

int qwen_tts_codec_stream_begin(qwen_tts_ctx_t *ctx, int max_frames) {
    if (!ctx || !ctx->hip) return -1;
    return qtts_dev_codec_stream_begin((qtts_dev_t *)ctx->hip, max_frames);
}

int qwen_tts_codec_stream_push(qwen_tts_ctx_t *ctx, const int *codes, int time_steps, float *out) {
    if (!ctx || !ctx->hip || !codes || !out || time_steps < 1) return -1;
    return qtts_dev_codec_stream_push_host((qtts_dev_t *)ctx->hip, codes, time_steps, out);
}

int qwen_tts_last_codes(qwen_tts_ctx_t *ctx, int *codes, int max_frames) {
    if (!ctx || !ctx->last_codes) return 0;
    int n = ctx->last_frames < max_frames ? ctx->last_frames : max_frames;
    memcpy(codes, ctx->last_codes, (size_t)n * ctx->config.num_code_groups * sizeof(int));
    return n;
}

int qwen_tts_last_codes_slot(qwen_tts_ctx_t *ctx, int slot, int *codes, int max_frames) {
    if (!ctx || !ctx->hip || slot < 0 || max_frames < 0) return -1;
    if (slot == 0) return qwen_tts_last_codes(ctx, codes, max_frames);
    return qtts_dev_get_codes((qtts_dev_t *)ctx->hip, slot, codes, max_frames);
}

/* -------------------------------------------------- stage functions (host) */
void qwen_tts_talker_prefill(qwen_tts_ctx_t *ctx, const float *input_embeds, int seq_len) {
    if (qtts_dev_talker_prefill_host((qtts_dev_t *)ctx->hip, input_embeds, seq_len, ctx->tk_x) != 0) {
        fprintf(stderr, "Error: talker prefill failed\n");
        return;
    }
    ctx->talker_kv_len = seq_len;
    if (qwen_tts_verbose >= 1) fprintf(stderr, "Talker prefill complete: %d tokens\n", seq_len);
}

void qwen_tts_talker_forward(qwen_tts_ctx_t *ctx, const float *input_embed, float *logits) {
    if (qtts_dev_talker_forward_host((qtts_dev_t *)ctx->hip, input_embed, logits, ctx->tk_x) != 0) {
        fprintf(stderr, "Error: talker forward failed\n");
        return;
    }
    ctx->talker_kv_len++;
}

void qwen_tts_subtalker_generate(qwen_tts_ctx_t *ctx, const float *talker_hidden, int first_code, int *out_codes) {
    qtts_gen_params_t gp;
    params_of(ctx, &gp);
    qtts_dev_t *dev = (qtts_dev_t *)ctx->hip;
    /* keep the device's sampling parameters in sync with the ctx fields */
    if (qtts_dev_begin(dev, 1, ctx->max_new_tokens > 0 ? ctx->max_new_tokens : 1, 16, &gp) != 0 ||
        qtts_dev_subtalker_host(dev, talker_hidden, first_code, out_codes) != 0)
        fprintf(stderr, "Error: sub-talker failed\n");
}

float *qwen_tts_codec_decode(qwen_tts_ctx_t *ctx, const int *codes, int time_steps, int *out_samples) {
    if (!ctx || !codes || !out_samples || time_steps <= 0) {
        if (out_samples) *out_samples = 0;
        return NULL;
    }
    codec_log_begin(ctx, time_steps);
    float *w = qtts_dev_codec_decode_host((qtts_dev_t *)ctx->hip, codes, time_steps, out_samples);
    codec_log_end(ctx, w ? *out_samples : 0);
    return w;
}

int qwen_tts_talker_hidden(qwen_tts_ctx_t *ctx, float *out) {
    if (!ctx || !ctx->tk_x) return -1;
    memcpy(out, ctx->tk_x, ctx->config.talker_hidden * sizeof(float));
    return 0;
}

/* ABI self-check for FFI bindings (tests/test_host.py compares this with the
 * ctypes mirror of qwen_tts_ctx_t) */
size_t qwen_tts_abi_sizeof_ctx(void) { return sizeof(qwen_tts_ctx_t); }
