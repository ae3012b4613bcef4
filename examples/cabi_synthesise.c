/* Plain-C host of text -> mel on the C ABI (include/stabletts_hip.h): no Python, no torch, no C++.
 *
 *   gcc -O2 -std=c99 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/cabi_synthesise.c \
 *       -L stabletts_amd -lstabletts_hip -L /opt/rocm/lib -lamdhip64 -Wl,-rpath,'$ORIGIN/../stabletts_amd' -o examples/cabi_synthesise
 *   examples/cabi_synthesise <inputs.bin> <mel_out.bin>
 *
 * StableTTS.synthesise (models/model.py:79-108) with the 31M configuration: MelStyleEncoder -> TextEncoder ->
 * DurationPredictor -> st_durations / st_align -> st_cfm_solve (Euler, CFG).  inputs.bin is a list of named tensors:
 *   "STSY" | uint32 count | count x { uint32 name_len | name | uint32 dtype (0 f32, 1 i64) | uint32 ndim | int64 shape[ndim] | data }
 * Names "se.*", "te.*", "dp.*", "dec.*" are the parameters of the four handles under their reference names; the inputs
 * are "in.x" (B, Tx) i64 token ids, "in.x_lengths" (B) i64, "in.y" (B, n_mels, T_ref) reference mel, "in.fake_speaker"
 * (1, gin), "in.fake_content" (1, n_mels, 1), "in.z" (B, n_mels, Ty) the decoder's start noise and "in.params"
 * (n_steps, cfg_strength, length_scale) f32.  Writes the mel (B, n_mels, Ty) as raw fp32 to mel_out.bin and prints
 *   cabi_synthesise B=.. Tx=.. Ty=.. y_lengths=a,b,.. sum=<double> abs=<double> finite=<0|1>
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "stabletts_hip.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 2; } } while (0)
#define ST(e, x) do { int r_ = (x); if (r_ != ST_OK) { fprintf(stderr, "st error %d: %s (%s:%d)\n", r_, st_last_error(e), __FILE__, __LINE__); return 3; } } while (0)

enum { N_VOCAB = 401, M = 128, HID = 256, FILT = 1024, HEADS = 4, ENC_LAYERS = 3, DEC_LAYERS = 6, KS = 3, GIN = 256 };

typedef struct { char name[128]; int dtype, ndim; int64_t shape[4]; size_t n; void* host; } Tensor;

static Tensor* g_t = NULL;
static uint32_t g_n = 0;

static int read_inputs(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 1; }
    char magic[4];
    if (fread(magic, 1, 4, f) != 4 || memcmp(magic, "STSY", 4) != 0 || fread(&g_n, 4, 1, f) != 1 || g_n > 4096) { fclose(f); return 1; }
    g_t = (Tensor*)calloc(g_n, sizeof(Tensor));
    for (uint32_t i = 0; i < g_n; ++i) {
        Tensor* t = &g_t[i];
        uint32_t len, dt, nd;
        if (fread(&len, 4, 1, f) != 1 || len >= sizeof(t->name) || fread(t->name, 1, len, f) != len) { fclose(f); return 1; }
        if (fread(&dt, 4, 1, f) != 1 || fread(&nd, 4, 1, f) != 1 || dt > 1 || nd < 1 || nd > 4) { fclose(f); return 1; }
        t->dtype = (int)dt; t->ndim = (int)nd; t->n = 1;
        if (fread(t->shape, 8, nd, f) != nd) { fclose(f); return 1; }
        for (uint32_t k = 0; k < nd; ++k) { if (t->shape[k] < 1) { fclose(f); return 1; } t->n *= (size_t)t->shape[k]; }
        const size_t bytes = t->n * (dt ? 8 : 4);
        t->host = malloc(bytes);
        if (!t->host || fread(t->host, 1, bytes, f) != bytes) { fclose(f); return 1; }
    }
    fclose(f);
    return 0;
}

static const Tensor* find(const char* name) {
    for (uint32_t i = 0; i < g_n; ++i) if (strcmp(g_t[i].name, name) == 0) return &g_t[i];
    fprintf(stderr, "missing tensor %s\n", name);
    return NULL;
}

static void* to_dev(const Tensor* t) {
    void* d = NULL;
    const size_t bytes = t->n * (t->dtype ? 8 : 4);
    if (hipMalloc(&d, bytes) != hipSuccess || hipMemcpy(d, t->host, bytes, hipMemcpyHostToDevice) != hipSuccess) return NULL;
    return d;
}

/* every tensor named <prefix><reference name> goes to handle e; then st_finalize */
static int load_params(st_engine* e, const char* prefix) {
    const size_t pl = strlen(prefix);
    int loaded = 0;
    for (uint32_t i = 0; i < g_n; ++i) {
        const Tensor* t = &g_t[i];
        if (strncmp(t->name, prefix, pl) != 0 || t->dtype != 0) continue;
        void* d = to_dev(t);
        if (!d) { fprintf(stderr, "upload of %s failed\n", t->name); return 2; }
        ST(e, st_load_param(e, t->name + pl, (const float*)d, t->shape, t->ndim));
        CK(hipFree(d));
        ++loaded;
    }
    if (loaded != st_num_params(e)) { fprintf(stderr, "%s: %d of %d parameters in the file\n", prefix, loaded, st_num_params(e)); return 1; }
    ST(e, st_finalize(e));
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s <inputs.bin> <mel_out.bin>\n", argv[0]); return 1; }
    if (st_abi_version() != ST_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    if (read_inputs(argv[1])) { fprintf(stderr, "bad input file %s\n", argv[1]); return 1; }
    const Tensor *tx = find("in.x"), *tl = find("in.x_lengths"), *ty = find("in.y"), *tfs = find("in.fake_speaker"),
                 *tfc = find("in.fake_content"), *tz = find("in.z"), *tp = find("in.params");
    if (!tx || !tl || !ty || !tfs || !tfc || !tz || !tp) return 1;
    const int B = (int)tx->shape[0], Tx = (int)tx->shape[1], Tref = (int)ty->shape[2];
    if (tx->dtype != 1 || tl->dtype != 1 || tl->n != (size_t)B || ty->shape[0] != B || ty->shape[1] != M || tz->ndim != 3 || tp->n != 3) {
        fprintf(stderr, "input shapes do not match the 31M configuration\n");
        return 1;
    }
    const float* prm = (const float*)tp->host;
    const int n_steps = (int)prm[0];
    const float cfg_strength = prm[1], length_scale = prm[2];

    /* the four handles, as models/model.py:36-40 builds the modules */
    st_engine *se = NULL, *te = NULL, *dp = NULL, *dec = NULL;
    const st_style_encoder_config se_cfg = {M, 128, GIN, 5, 2};
    const st_config te_cfg = {M, HID, FILT, HEADS, ENC_LAYERS, KS, GIN, ST_OPERAND_F16};
    const st_duration_predictor_config dp_cfg = {HID, FILT, KS, GIN};
    const st_config dec_cfg = {M, HID, FILT, HEADS, DEC_LAYERS, KS, GIN, ST_OPERAND_F16};
    if (st_create_style_encoder(&se_cfg, 0, &se) || st_create_text_encoder(&te_cfg, N_VOCAB, 0, &te) ||
        st_create_duration_predictor(&dp_cfg, 0, &dp) || st_create(&dec_cfg, 0, &dec)) {
        fprintf(stderr, "create: %s\n", st_last_error(NULL));
        return 1;
    }
    int rc;
    if ((rc = load_params(se, "se.")) || (rc = load_params(te, "te.")) || (rc = load_params(dp, "dp.")) || (rc = load_params(dec, "dec."))) return rc;

    hipStream_t s; CK(hipStreamCreate(&s));
    void *x = to_dev(tx), *xl = to_dev(tl), *y = to_dev(ty), *fs = to_dev(tfs), *fc = to_dev(tfc), *z = to_dev(tz);
    if (!x || !xl || !y || !fs || !fc || !z) { fprintf(stderr, "upload failed\n"); return 2; }
    float *c, *h, *mu_x, *x_mask, *logw, *w_ceil, *cum; int64_t* y_lengths;
    CK(hipMalloc((void**)&c, (size_t)B * GIN * 4));
    CK(hipMalloc((void**)&h, (size_t)B * HID * Tx * 4));
    CK(hipMalloc((void**)&mu_x, (size_t)B * M * Tx * 4));
    CK(hipMalloc((void**)&x_mask, (size_t)B * Tx * 4));
    CK(hipMalloc((void**)&logw, (size_t)B * Tx * 4));
    CK(hipMalloc((void**)&w_ceil, (size_t)B * Tx * 4));
    CK(hipMalloc((void**)&cum, (size_t)B * Tx * 4));
    CK(hipMalloc((void**)&y_lengths, (size_t)B * 8));

    ST(se, st_style_encoder_forward(se, (const float*)y, NULL, c, B, Tref, s));                                  /* model.py:79 */
    ST(te, st_text_encoder_forward(te, (const int64_t*)x, (const int64_t*)xl, c, h, mu_x, x_mask, B, Tx, s));    /* :80 */
    ST(dp, st_duration_predictor_forward(dp, h, x_mask, c, logw, B, Tx, s));                                      /* :81 */
    ST(NULL, st_durations(logw, x_mask, length_scale, B, Tx, w_ceil, cum, y_lengths, s));                         /* :83-85 */
    int64_t* yl = (int64_t*)malloc((size_t)B * 8);
    CK(hipMemcpyAsync(yl, y_lengths, (size_t)B * 8, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));                    /* y_lengths.max() sizes the mel tensors, as at model.py:86 */
    int Ty = 0;
    for (int b = 0; b < B; ++b) if (yl[b] > Ty) Ty = (int)yl[b];
    if (tz->shape[0] != B || tz->shape[1] != M || tz->shape[2] != Ty) {
        fprintf(stderr, "in.z is (%lld, %lld, %lld), the durations give Ty = %d\n", (long long)tz->shape[0], (long long)tz->shape[1],
                (long long)tz->shape[2], Ty);
        return 5;
    }
    const size_t nmel = (size_t)B * M * Ty;
    float *mu_y, *y_mask, *mel;
    CK(hipMalloc((void**)&mu_y, nmel * 4));
    CK(hipMalloc((void**)&y_mask, (size_t)B * Ty * 4));
    CK(hipMalloc((void**)&mel, nmel * 4));
    ST(NULL, st_align(cum, x_mask, y_lengths, mu_x, B, M, Tx, Ty, NULL, mu_y, y_mask, s));                         /* :87-95 */
    ST(dec, st_cfm_solve(dec, mu_y, y_mask, (const float*)z, c, n_steps, ST_SOLVER_EULER, 1, cfg_strength,
                         (const float*)fs, (const float*)fc, mel, B, Ty, s));                                     /* :98-102 */
    float* out = (float*)malloc(nmel * 4);
    CK(hipMemcpyAsync(out, mel, nmel * 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));

    double sum = 0.0, asum = 0.0; int finite = 1;
    for (size_t i = 0; i < nmel; ++i) {
        sum += out[i]; asum += out[i] < 0 ? -out[i] : out[i];
        if (!(out[i] == out[i]) || out[i] > 1e30f || out[i] < -1e30f) finite = 0;
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(out, 4, nmel, f) != nmel) { fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    fclose(f);
    printf("cabi_synthesise B=%d Tx=%d Ty=%d y_lengths=", B, Tx, Ty);
    for (int b = 0; b < B; ++b) printf(b ? ",%lld" : "%lld", (long long)yl[b]);
    printf(" sum=%.9e abs=%.9e finite=%d\n", sum, asum, finite);
    st_destroy(se); st_destroy(te); st_destroy(dp); st_destroy(dec);
    return finite ? 0 : 4;
}
