// towers_trace.hip -- the tower orchestration as a call trace, on the CPU: every launcher towers.hip calls is a stub that prints its name,
// the current ProfRegion and every argument; the driver walks every branch of the five entry points with fake (never dereferenced)
// pointers.  Build against the towers.o of two commits and cmp the outputs: what a host-side refactor must leave identical
// (profiles/r08_towers_refactor.md).
//   hipcc --offload-arch=gfx950 -std=c++17 -Ivtc_amd/csrc -Iinclude -c tools/probes/towers_trace.hip -o towers_trace.o && hipcc --offload-arch=gfx950 -o towers_trace towers_trace.o build/obj/towers.o
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include <vector>
#include "common.h"

static int g_region = 0, g_gather = 0, g_fused = 0;
template <class T> void pr(T v) {
  if constexpr (std::is_pointer_v<T>) printf(" %p", (const void *)v);
  else if constexpr (std::is_floating_point_v<T>) printf(" %g", (double)v);
  else printf(" %lld", (long long)v);
}
template <class... A> int LOG(const char *name, A... a) { printf("%s r%d", name, g_region); (pr(a), ...); printf("\n"); return 0; }

ProfRegion::ProfRegion(int region) { prev_ = g_region; g_region = region; }
ProfRegion::~ProfRegion() { g_region = prev_; }
namespace vtcgemm { int num_cus() { return 256; } }

int launch_gemm(const void *A, const void *W, const float *bias, void *out, int M, int N, int K, int dtype, const GemmEpi &e, hipStream_t s) {
  return LOG("gemm", A, W, bias, out, M, N, K, dtype, s, e.mode, e.out_dtype, e.skip_mod, e.pos, e.temporal, e.P, e.F, e.T, e.frames_major, e.gather,
             e.grid, e.res, e.patch, e.ldo, e.y16, e.y16lo, e.fold_part, e.fold_stat, e.fold_s, e.m_dev, e.ksplit, e.split_stride, e.ln_g, e.ln_out);
}
bool gemm_patch_gather_supported(int a, int b, int c, int d, int pixel_dtype, int dtype) { return g_gather == 1 || (g_gather == 2 && pixel_dtype == dtype); }
int launch_layernorm(const float *x, const float *g, const float *b, void *y, int rows, int width, int od, const int *ri, int rm, bool nn, hipStream_t s, const int *rd) { return LOG("layernorm", x, g, b, y, rows, width, od, ri, rm, nn, s, rd); }
int launch_fold_stats(const float *part, int nb, int rows, float *stat, hipStream_t s, const int *rd) { return LOG("fold_stats", part, nb, rows, stat, s, rd); }
int launch_ln_cast_rowstats(const float *x, const float *g, const float *b, void *y, void *yl, float *st, int rows, int w, int dt, hipStream_t s) { return LOG("ln_cast_rowstats", x, g, b, y, yl, st, rows, w, dt, s); }
int launch_splitk_resid_rows(const float *part, int nsl, int stride, const float *bias, void *hi, void *lo, float *stat, int rows, int width, int dtype, hipStream_t s, const int *rd) { return LOG("splitk_resid_rows", part, nsl, stride, bias, hi, lo, stat, rows, width, dtype, s, rd); }
int launch_cast_rowstats(const float *x, void *y, void *yl, float *st, int rows, int w, int dt, hipStream_t s, const int *rd) { return LOG("cast_rowstats", x, y, yl, st, rows, w, dt, s, rd); }
int launch_gather_rows(const void *src, void *dst, int n, int rb, const int *ri, int rm, hipStream_t s) { return LOG("gather_rows", src, dst, n, rb, ri, rm, s); }
int launch_split_merge_rows(const void *hi, const void *lo, float *x, int n, int w, const int *ri, int rm, int dt, hipStream_t s, const int *rd) { return LOG("split_merge_rows", hi, lo, x, n, w, ri, rm, dt, s, rd); }
int launch_single_query_attention(const void *qkv, const void *q, float *out, int n_out, int L, int heads, int s2, int a0, int a1, int a2, int a3, int ps, const int *eot, const int *offs, int ctx, int dt, hipStream_t s) { return LOG("sq_attention", qkv, q, out, n_out, L, heads, s2, a0, a1, a2, a3, ps, eot, offs, ctx, dt, s); }
int launch_mean_cast(const float *x, void *out, int n, int F, int W, int dt, hipStream_t s) { return LOG("mean_cast", x, out, n, F, W, dt, s); }
int launch_attention(const void *qkv, void *out, float *cls, int n_seq, int L, int heads, int causal, int s2, int a0, int a1, int a2, int a3, int ps, int dt, hipStream_t s) { return LOG("attention", qkv, out, cls, n_seq, L, heads, causal, s2, a0, a1, a2, a3, ps, dt, s); }
int launch_im2row(const void *px, int pd, void *out, int dt, int nf, int grid, int patch, int res, const float *mean, const float *stdv, hipStream_t s) { return LOG("im2row", px, pd, out, dt, nf, grid, patch, res, s); }
int patch_k_padded(int patch) { return (3 * patch * patch + 63) / 64 * 64; }
int launch_pixels_u8_to_operand(const void *px, void *out, int dt, int nf, int res, const float *mean, const float *stdv, hipStream_t s) { return LOG("u8_to_operand", px, out, dt, nf, res, s); }
int launch_cls_rows(float *x, const float *cls, const float *pos0, int n, int T, int W, hipStream_t s) { return LOG("cls_rows", x, cls, pos0, n, T, W, s); }
int launch_cls_mean(const float *ct, void *out, int dt, int n, int F, int T, int W, hipStream_t s) { return LOG("cls_mean", ct, out, dt, n, F, T, W, s); }
int launch_text_prep(const TextIds &ids, int n, int ctx, int *lens, int *offs, int *m, hipStream_t s) { return LOG("text_prep", ids.a, ids.b, ids.n_a, ids.n_b, n, ctx, lens, offs, m, s); }
int launch_text_embed(const TextIds &ids, const float *tok, const float *pos, float *x, int *eot, int n, int ctx, int W, int vocab, hipStream_t s) { return LOG("text_embed", ids.a, ids.b, ids.n_a, ids.n_b, tok, pos, x, eot, n, ctx, W, vocab, s); }
int launch_text_embed_ragged(const TextIds &ids, const float *tok, const float *pos, const int *so, float *x, int *eot, int n, int ctx, int W, int vocab, hipStream_t s) { return LOG("text_embed_ragged", ids.a, ids.b, ids.n_a, ids.n_b, tok, pos, so, x, eot, n, ctx, W, vocab, s); }
int launch_attention_ragged(const void *qkv, void *out, int n, int maxL, int heads, int causal, const int *so, double flops, const int *rd, int dt, hipStream_t s) { return LOG("attention_ragged", qkv, out, n, maxL, heads, causal, so, flops, rd, dt, s); }
int launch_attention_generic_small(const void *qkv, void *out, int n, int L, int heads, int hd, int dt, hipStream_t s) { return LOG("attention_generic_small", qkv, out, n, L, heads, hd, dt, s); }
int launch_cam_tokens(const float *m, const float *c, const int64_t *cm, const float *me, const float *aux, float *X, int B, int nc, int na, int ctx, int D, hipStream_t s) { return LOG("cam_tokens", m, c, cm, me, aux, X, B, nc, na, ctx, D, s); }
int launch_cls_global_attention(const void *qkv, void *out, int n, int T, int heads, int dt, hipStream_t s) { return LOG("cls_global_attention", qkv, out, n, T, heads, dt, s); }
int launch_cam_finalize(const float *Y, const float *lin, const float *mf, float *out, int B, int Lc, int D, int ifa, int act, float sc, const float *bm, const float *bv, hipStream_t s) { return LOG("cam_finalize", Y, lin, mf, out, B, Lc, D, ifa, act, sc, bm, bv, s); }
bool cam_fused_supported(const vtc_cam_w *w, int B, int nc, int na, int dtype) { return g_fused != 0; }
size_t cam_fused_bar_bytes() { return 1000; }
int launch_cam_fused(const vtc_cam_w *w, const float *m, const float *c, const int64_t *cm, const float *aux, int ctx, int B, int nc, int na, float *ad, float *x, float *big, float *att, int *bar, hipStream_t s) {
  LOG("cam_fused", m, c, cm, aux, ctx, B, nc, na, ad, x, big, att, bar, s);
  return g_fused == 1 ? 0 : -1;
}

// ---- driver ------------------------------------------------------------------------------------------------------------------
static uintptr_t g_next = 0x10000;
template <class T> const T *fake() { g_next += 0x1000; return (const T *)g_next; }
static std::vector<vtc_block_w> blocks(int layers, bool tsf, bool tout, int fold /* 0 none, 1 all, 2 all but layer 1's fc */) {
  std::vector<vtc_block_w> v(layers);
  for (int l = 0; l < layers; ++l) {
    vtc_block_w &b = v[l];
    memset(&b, 0, sizeof b);
    b.ln1_g = fake<float>(); b.ln1_b = fake<float>(); b.qkv_w = fake<void>(); b.qkv_b = fake<float>(); b.out_w = fake<void>(); b.out_b = fake<float>();
    b.ln2_g = fake<float>(); b.ln2_b = fake<float>(); b.fc_w = fake<void>(); b.fc_b = fake<float>(); b.proj_w = fake<void>(); b.proj_b = fake<float>();
    if (tsf) {
      b.lnt_g = fake<float>(); b.lnt_b = fake<float>(); b.tqkv_w = fake<void>(); b.tqkv_b = fake<float>();
      if (tout) { b.tout_w = fake<void>(); b.tout_b = fake<float>(); }
      b.tfc_w = fake<void>(); b.tfc_b = fake<float>();
    }
    if (fold) {
      b.qkv_wf = fake<void>(); b.qkv_s = fake<float>(); b.qkv_c = fake<float>();
      if (!(fold == 2 && l == 1)) { b.fc_wf = fake<void>(); b.fc_s = fake<float>(); b.fc_c = fake<float>(); }
      if (tsf) { b.tqkv_wf = fake<void>(); b.tqkv_s = fake<float>(); b.tqkv_c = fake<float>(); }
    }
  }
  return v;
}
int main() {
  void *ws = (void *)0x100000000ull, *st = (void *)0x77;
  float *out = (float *)0x200000000ull;
  const size_t big = (size_t)1 << 40;
  const int flagsets[] = {0, VTC_TOWER_FULL_LAST_LAYER, VTC_TOWER_NO_LN_FOLD, VTC_TOWER_NO_SPLITK, VTC_TOWER_FULL_LAST_LAYER | VTC_TOWER_NO_LN_FOLD | VTC_TOWER_NO_SPLITK};
  const int dts[] = {VTC_F32, VTC_BF16, VTC_F16};
  int cases = 0;
  for (int width : {128, 256, 768})
    for (int layers : {0, 1, 2})
      for (int fold : width == 256 ? std::vector<int>{0, 1, 2} : std::vector<int>{1})
        for (int flags : flagsets)
          for (int dt : dts) {
            // vision: image, alt (with / without a separate out_proj), v1
            for (int kind = 0; kind < 4; ++kind) {
              const bool tsf = kind > 0;
              g_next = 0x10000;
              auto bl = blocks(layers, tsf, kind >= 2, fold);
              vtc_vision_w w;
              memset(&w, 0, sizeof w);
              w.width = width; w.heads = width / 64; w.layers = layers; w.patch = 32; w.embed_dim = 128; w.nframes = tsf ? 8 : 0;
              w.variant = kind == 3; w.flags = flags; w.conv_w = fake<void>(); w.class_embedding = fake<float>(); w.pos = fake<float>();
              w.temporal = tsf ? fake<float>() : nullptr; w.ln_pre_g = fake<float>(); w.ln_pre_b = fake<float>(); w.ln_post_g = fake<float>();
              w.ln_post_b = fake<float>(); w.proj_t = fake<float>(); w.blocks = bl.data();
              for (int grid : {2, 7})
                for (int n : {1, 3, 100}) {
                  if (grid == 7 && n == 100 && width != 256) continue;
                  for (int F : tsf ? std::vector<int>{1, 4} : std::vector<int>{1})
                    for (int pd : (n == 100 && grid == 7) ? std::vector<int>{VTC_F32, VTC_U8, VTC_BF16} : std::vector<int>{VTC_F32}) {
                      for (g_gather = 0; g_gather < ((n == 100 && grid == 7) ? 3 : 1); ++g_gather) {
                        w.grid = grid;
                        printf("== vision kind %d W %d layers %d fold %d flags %d dt %d grid %d n %d F %d pd %d gather %d: ws %zu\n", kind, width, layers, fold, flags, dt, grid, n, F, pd, g_gather,
                               vtc_vision_workspace_bytes(&w, n, F, dt));
                        const int rc = vtc_vision_forward(&w, (const void *)0x300000000ull, pd, n, F, out, ws, big, dt, st);
                        printf("rc %d %s\n", rc, rc ? vtc_last_error() : "");
                        ++cases;
                      }
                      g_gather = 0;
                    }
                }
            }
            // text: dense, dense two arrays, device offsets (one / two arrays), host offsets; half_layers 0 / 1 / all
            for (int half : {0, 1, 99}) {
              if (half && dt != VTC_BF16) continue;
              g_next = 0x10000;
              auto bl = blocks(layers, false, false, fold);
              vtc_text_w w;
              memset(&w, 0, sizeof w);
              w.width = width; w.heads = width / 64; w.layers = layers; w.ctx = 24; w.vocab = 49408; w.embed_dim = 128; w.half_layers = half > layers ? layers : half;
              w.flags = flags; w.tok_emb = fake<float>(); w.pos = fake<float>(); w.ln_final_g = fake<float>(); w.ln_final_b = fake<float>();
              w.proj_t = fake<float>(); w.blocks = bl.data();
              const int64_t *ia = (const int64_t *)0x400000000ull, *ib = (const int64_t *)0x500000000ull;
              for (int n : {1, 3, 50}) {
                printf("== text W %d layers %d fold %d flags %d dt %d half %d n %d: ws %zu %zu\n", width, layers, fold, flags, dt, half, n, vtc_text_workspace_bytes(&w, n, dt),
                       vtc_text_ragged_workspace_bytes(&w, n, n * 11, dt));
                int rc = vtc_text_forward(&w, ia, n, out, ws, big, dt, st);
                printf("rc %d\n", rc);
                for (int ragged = 0; ragged < 2; ++ragged)
                  for (int nb : {0, 2}) {
                    rc = vtc_text_forward2(&w, ia, n, nb ? ib : nullptr, nb, ragged, out, ws, big, dt, st);
                    printf("rc %d\n", rc);
                    ++cases;
                  }
                rc = vtc_text_forward_ragged(&w, ia, n, (const int *)0x600000000ull, n * 11, out, ws, big, dt, st);
                printf("rc %d\n", rc);
                cases += 2;
              }
            }
            // CAM (fold / flags do not reach it: once per (width, layers, dt))
            if (fold == 0 && flags == 0 && dt != VTC_F16) {
              g_next = 0x10000;
              auto bl = blocks(layers, false, false, 1);
              vtc_cam_w w;
              memset(&w, 0, sizeof w);
              w.width = width; w.layers = layers; w.squash_scale = 1.f; w.final_linear = fake<void>(); w.mask_embedding = fake<float>(); w.blocks = bl.data();
              for (int heads : {width / 64, 8})
                for (int ifa = 0; ifa < 2; ++ifa)
                  for (int B : {1, 3})
                    for (int na : {0, 2})
                      for (g_fused = 0; g_fused < 3; ++g_fused) {
                        w.heads = heads; w.init_from_avg = ifa;
                        printf("== cam W %d layers %d dt %d heads %d ifa %d B %d na %d fused %d: ws %zu %zu\n", width, layers, dt, heads, ifa, B, na, g_fused,
                               vtc_cam_workspace_bytes(&w, B, 5, dt), vtc_cam_aux_workspace_bytes(&w, B, 5, na, dt));
                        const int rc = na ? vtc_cam_forward_aux(&w, (const float *)0x700000000ull, (const float *)0x800000000ull, (const int64_t *)0x400000000ull, (const float *)0x900000000ull, 24, B, 5, na, out, ws, big, dt, st)
                                          : vtc_cam_forward(&w, (const float *)0x700000000ull, (const float *)0x800000000ull, (const int64_t *)0x400000000ull, 24, B, 5, out, ws, big, dt, st);
                        printf("rc %d %s\n", rc, rc ? vtc_last_error() : "");
                        ++cases;
                      }
              g_fused = 0;
            }
          }
  fprintf(stderr, "%d cases\n", cases);
  return 0;
}
