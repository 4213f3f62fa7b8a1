// many_common.h -- what the MFMA passes over a half gallery share (search_many.hip: the nearest `depth`; range_many.hip: every row within a
// radius).  One copy of each piece, so that the passes cannot drift: both multiply the same operands, form the same approximate distance
// A and bound it by the same eps.  In the order of the file:
//   the bound            many_kappa, many_eps and their derivation
//   the query prologue   many_prep_kernel, the layout of the B-fragment image it writes, its four workspace regions and its launch
//   an item              many_load_frags (the A fragments of NKS MFMA steps of a tile, straight from global memory), ManyImage (the B
//                        fragments of a wave in the LDS), many_multiply (the hi and lo products and the row norm)
//   the epilogue         many_row_norm, many_dist: |g|^2 of a tile's rows and A of a pair
//   the walk             many_walk: which units a workgroup takes, what it skips, what is loaded ahead of what
//   the host side        workgroups a CU, the image's LDS bytes, the (MASKED, NKS) instantiation of a call
// A pass kernel is the prologue of the lane's query, its own epilogue (a list insertion, or the band decision and the hit word), one call
// of the walk, and its stores.
#pragma once
#include "search_walk.h"

namespace {
using namespace vtcsweep;

constexpr int MANY_MAX_Q = 64;         // queries of a call at most: four waves of 16
constexpr int MANY_KC = 512;           // columns of a K chunk: 16 MFMA steps, 32 KB of B fragments a wave
constexpr int MANY_KS = MANY_KC / 32;
constexpr int QF_DEAD = 1, QF_FALLBACK = 2;

typedef _Float16 half2_t __attribute__((ext_vector_type(2)));

// THE BOUND.  A(q, j) = fl(fl(qn + gn) - 2 acc / s) with qn, gn the fp32 squared norms and acc the MFMA's fp32 sum over k of
// g_k hi_k + g_k lo_k, where x = s q, hi = fl16(x), lo = fl16(x - hi) and s = 2^(13 - e) puts the largest |x_k| into [2^13, 2^14)
// (scaling by a power of two is exact).  With u = 2^-24, S = |q|^2 + |g|^2, |q||g| <= S / 2:
//   split      x_k - hi_k is exact in fp32 and |x_k - hi_k - lo_k| <= 2^-22 |x_k| while hi_k and lo_k are normal halves.  A subnormal one is
//              a component below 2^-27 of the largest; even if the matrix core FLUSHED a subnormal operand (it does not: the tests'
//              subnormal rows), that is an absolute 2^-13 per component, sum_k |g_k| 2^-13 <= 2^-13 sqrt(d) |g| <= 2^-20.5 |x||g| as
//              |x| >= 2^13 and d <= 2048.  Together < 2^-20 |q||g| on the dot product, 2^-20 S on the distance.
//   MFMA       2 d exact fp16 x fp16 products summed in fp32, in an order and with an internal rounding the hardware does not
//              promise: two units a term, 4 d u |q||g| on the dot product, 4 d u S on the distance.
//   norms      gn: d / 2 dot2 steps of two roundings and the two lane adds, qn: d fused steps and the butterfly: <= 2 d u S together.
//   epilogue   fl(qn + gn) and the final fused multiply-add, each one rounding of a value <= 2 S: <= 8 u S with slack.
//   range      acc / s, qn and the scaled components may UNDERFLOW for queries far below fp32's normal range: an absolute term far
//              above d 2^-149.  Overflow is not bounded but detected: a live row with a finite norm whose A is not finite is no
//              bounded pair (the search flags the query, the range pass decides the pair in fp64).
// So |A - D| <= many_eps(many_kappa(d), qn, gn) with many_kappa(d) = (6 d + 8) 2^-24 + 2^-20, for every pair whose A is finite and
// whose query is not QF_FALLBACK.  The search bounds a whole list at once, with gn the maximum over the LIVE rows with a FINITE norm (a
// row with a NaN / inf is never a candidate, and a dead one is never looked at); the range pass bounds each pair with the row's own.
// One expression in fp64, in one order: the queries it sends to the fallback and the pairs it sends to the band are observable.
inline float many_kappa(int d) { return (6.0f * d + 8.0f) / 16777216.0f + 1.0f / 1048576.0f; }
__host__ __device__ inline double many_eps(float kappa, float qn, float gn) {
  return (double)kappa * ((double)qn + (double)gn) * (1.0 + 1e-6) + 1e-35;
}

inline int many_qgroups(int nq) { return cdiv(nq, 16); }
// The B-fragment image of the queries: uint4 [qgroups][d / 32][hi, lo][64 lanes].  The fragment of MFMA step ks: lane (kq, u) = 16 kq + u
// holds the 8 halves k = 32 ks + 8 kq .. + 7 of query u of the group.
inline size_t many_img_bytes(int nq, int d) { return (size_t)many_qgroups(nq) * 16 * d * 2 * sizeof(_Float16); }
__device__ __forceinline__ size_t many_img_at(int grp, int d, int ks, int kq, int u) {      // of the hi fragment; lo is 64 further
  return ((size_t)(grp * (d / 32) + ks) * 2) * 64 + kq * 16 + u;
}
// MFMA steps of an item of a pass: the largest of 16, 8, 4, 2 that divides the row's d / 32 (d % 64 == 0: that is even)
inline int many_item_steps(int d) {
  const int ksteps = d / 32;
  return ksteps % 16 == 0 ? 16 : (ksteps % 8 == 0 ? 8 : (ksteps % 4 == 0 ? 4 : 2));
}

// One wave per query slot (16 x qgroups of them; a slot past the last query is a dead row of zeros, as a query with a NaN / inf is).
// Zeroes the call's counter, `counter_words` int32 of it.
__global__ __launch_bounds__(64) void many_prep_kernel(const float *__restrict__ queries, int nq, int d, uint4 *__restrict__ qimg,
                                                       float *__restrict__ qn, float *__restrict__ inv_s, int *__restrict__ qflag,
                                                       int *__restrict__ counter, int counter_words, int *__restrict__ nonfinite) {
  const int q = blockIdx.x, lane = threadIdx.x;
  if (q == 0 && lane < counter_words) counter[lane] = 0;
  const float *row = queries + (size_t)min(q, nq - 1) * d;
  float m = 0.f, n2 = 0.f;
  bool bad = false;
  for (int c = lane * 4; c < d; c += 256) {
    const float4 v = *reinterpret_cast<const float4 *>(row + c);
    bad = bad || !(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w));
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    n2 = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, n2))));
  }
  const bool nonfin = __ballot(bad) != 0, dead = nonfin || q >= nq;
  m = wave_max(dead ? 0.f : m);
  n2 = wave_sum(n2);
  int flag = dead ? QF_DEAD : 0, e = 13;                   // m == 0: s = 1
  if (m > 0.f) e = ilogbf(m);
  int se = 13 - e;                                         // s = 2^se puts m into [2^13, 2^14)
  if (se > 126) {                                          // a query below 2^-113: s would leave fp32, the split has no bound
    se = 126;
    flag |= QF_FALLBACK;
  }
  const float s = __int_as_float((se + 127) << 23);
  if (lane == 0) {
    qn[q] = dead ? 0.f : n2;
    inv_s[q] = __int_as_float((127 - se) << 23);
    qflag[q] = flag;
    if (nonfin && q < nq && nonfinite) atomicOr(nonfinite, 2);
  }
  const int grp = q >> 4, u = q & 15;
  for (int b = lane; b < d / 8; b += 64) {
    f16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = dead ? 0.f : row[b * 8 + j] * s;
      hi[j] = (_Float16)x;
      lo[j] = (_Float16)(x - (float)hi[j]);
    }
    const size_t o = many_img_at(grp, d, b >> 2, b & 3, u);
    qimg[o] = __builtin_bit_cast(uint4, hi);
    qimg[o + 64] = __builtin_bit_cast(uint4, lo);
  }
}

// What the prologue writes, four regions of a pass's workspace in this order, and its launch.  `counter`: see many_prep_kernel.
struct ManyPrologue {
  uint4 *qimg;          // [qgroups][d / 32][hi, lo][64 lanes]: B fragments
  float *qn, *inv_s;    // [64]
  int *qflag;           // [64]
};
inline ManyPrologue many_prologue_ws(Bump &b, int nq, int d) {
  ManyPrologue p;
  p.qimg = (uint4 *)b.take(many_img_bytes(nq, d));
  p.qn = (float *)b.take(MANY_MAX_Q * sizeof(float));
  p.inv_s = (float *)b.take(MANY_MAX_Q * sizeof(float));
  p.qflag = (int *)b.take(MANY_MAX_Q * sizeof(int));
  return p;
}
inline void many_launch_prep(const float *queries, int nq, int d, const ManyPrologue &p, int *counter, int counter_words, int *nonfinite,
                             hipStream_t stream) {
  hipLaunchKernelGGL(many_prep_kernel, dim3(many_qgroups(nq) * 16), dim3(64), 0, stream, queries, nq, d, p.qimg, p.qn, p.inv_s, p.qflag, counter,
                     counter_words, nonfinite);
}

// ---- an item: NKS MFMA steps of a tile of 16 stored rows.  NKS is a template parameter: the loads of an item are then unconditional
// and the compiler counts them, so waiting for one item's fragments leaves the next item's in flight; d = 32 NKS nchunks.

// The A fragments of an item -- NKS MFMA steps of tile t, the 16 rows 16 t .. 16 t + 15: lane (kq, u) holds row u of the tile, halves
// 32 ks + 8 kq .. + 7 of chunk `chunk`, 16 bytes straight from global memory.  `bits`: the tile's rows that are live and inside the
// gallery, != 0.  A dead row (or one past the gallery) is pointed at a live row of the tile: its memory is not read, its results are
// dropped by the caller.
template <int NKS>
__device__ __forceinline__ void many_load_frags(const _Float16 *gallery, int d, long long t, int chunk, unsigned bits, int u, int kq,
                                                f16x8 (&ga)[NKS]) {
  const long long row = t * 16 + (((bits >> u) & 1) ? u : __ffs((int)bits) - 1);
  const _Float16 *p = gallery + (size_t)row * d + chunk * (NKS * 32) + kq * 8;
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) ga[ks] = *reinterpret_cast<const f16x8 *>(p + ks * 32);
}

// The B fragments of a wave's 16 queries in the LDS.  Up to MANY_KC columns the wave's whole image is RESIDENT, copied once at the
// kernel's start; a longer row keeps one item's part and reloads it per item, behind two barriers -- every wave of the workgroup walks
// the same items.  The waves' images lie one after the other from the start of the dynamic LDS.
__host__ __device__ constexpr int many_img_vecs(int d, int nks) { return (d <= MANY_KC ? d / 32 : nks) * 2 * 64; }      // uint4 of a wave
constexpr int MANY_IMG_MAX_BYTES = many_img_vecs(MANY_KC, MANY_KS) * (int)sizeof(uint4);                              // of a wave: 32 KB
template <int NKS>
struct ManyImage {
  uint4 *img;
  const uint4 *gimg;
  bool resident;
  // by every wave of the workgroup, at the kernel's start; ends in a barrier
  __device__ __forceinline__ ManyImage(uint4 *smem, const uint4 *qimg, int d, int wave, int lane)
      : img(smem + (size_t)wave * many_img_vecs(d, NKS)), gimg(qimg + (size_t)wave * (d / 32) * 2 * 64), resident(d <= MANY_KC) {
    if (resident)
      for (int x = lane; x < d / 32 * 2 * 64; x += 64) img[x] = gimg[x];
    __syncthreads();
  }
  // the lane's B fragments of chunk `chunk`: hi of step ks at [(2 ks) 64], lo at [(2 ks + 1) 64].  By every wave, once per item.
  __device__ __forceinline__ const uint4 *item(int chunk, int lane) const {
    if (!resident) {
      __syncthreads();
      for (int x = lane; x < NKS * 2 * 64; x += 64) img[x] = gimg[(size_t)chunk * NKS * 2 * 64 + x];
      __syncthreads();
    }
    return img + (resident ? chunk * NKS * 2 * 64 : 0) + lane;
  }
};

// The multiply step of an item: per MFMA step the hi and the lo product into acc (acc[i]: query u x row 4 kq + i of the tile), and the
// lane's share of |g|^2 of row u, from the fragment it holds, into nrm.
template <int NKS>
__device__ __forceinline__ void many_multiply(const f16x8 (&ga)[NKS], const uint4 *bi, f32x4 &acc, float &nrm) {
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const f16x8 bh = __builtin_bit_cast(f16x8, bi[(ks * 2) * 64]), bl = __builtin_bit_cast(f16x8, bi[(ks * 2 + 1) * 64]);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ga[ks], bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ga[ks], bl, acc, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const half2_t h = {ga[ks][2 * j], ga[ks][2 * j + 1]};
      nrm = __builtin_amdgcn_fdot2(h, h, nrm, false);
    }
  }
}

// ---- the epilogue of a tile, after its last chunk
// every lane: |g|^2 of row u of the tile, from the four kq lanes' shares
__device__ __forceinline__ float many_row_norm(float nrm) {
  nrm += __shfl_xor(nrm, 16, 64);
  return nrm + __shfl_xor(nrm, 32, 64);
}
// A of (the lane's query, a row): acc the pair's MFMA sum, qn and gn the squared norms, m2inv_s = -2 / s of the query
__device__ __forceinline__ float many_dist(float acc, float qn, float gn, float m2inv_s) { return fmaf(m2inv_s, acc, qn + gn); }

// ---- the walk of a pass kernel over the gallery, by every wave of the workgroup alike.  A UNIT is TILES tiles of 16 rows: one tile for
// the search, the two tiles of a hit word (32 rows) for the range pass.
//   * Workgroup b of G takes the units b, b + G, ...
//   * A unit with no live row inside the gallery goes to dead(w) BEFORE anything of it is loaded, and a dead tile of a live unit is
//     skipped, so every item that is loaded is multiplied: the loads of an item are unconditional (see NKS above).
//   * The mask word of a unit (its address is uniform: a scalar load, which the vector loads' counter does not see) is read one unit
//     ahead; only a run of dead units is searched word by word.  Without MASKED `live` is not looked at.
//   * Two fragment sets: the loads of the next item are in flight while this one is multiplied.  After the last item the loads are
//     issued once more for the item itself (a live tile) and dropped, which keeps their number fixed.
//   * compute(w, h, avail, chunk, frags) multiplies chunk `chunk` of tile h of unit w, whose fragments are `frags`, and after the last
//     chunk does the tile's epilogue.  avail: the unit's rows that are live and inside the gallery, tile h's 16 at bit 16 h, != 0.
//     Items arrive in ascending (w, h, chunk).
template <bool MASKED, int NKS, int TILES, typename Compute, typename Dead>
__device__ __forceinline__ void many_walk(const _Float16 *gallery, const unsigned *live, int ng, int d, int u, int kq, Compute compute, Dead dead) {
  static_assert(TILES == 1 || TILES == 2, "a unit's rows lie in one mask word");
  constexpr int ROWS = 16 * TILES;
  constexpr unsigned FULL = TILES == 2 ? 0xffffffffu : 0xffffu;
  const int nchunks = d / (32 * NKS);
  const long long n_units = ((long long)ng + ROWS - 1) / ROWS, G = gridDim.x;
  auto word_at = [&](long long w) -> unsigned {           // the mask bits of unit w, as loaded
    if constexpr (!MASKED) return FULL;
    if (w >= n_units) return 0;
    if constexpr (TILES == 2) return live[w];
    return live[w >> 1] >> ((w & 1) * 16);
  };
  auto avail_at = [&](long long w, unsigned word) -> unsigned {      // ... of its rows inside the gallery, wave-uniform; 0 past the end
    if (w >= n_units) return 0;
    const long long left = (long long)ng - w * ROWS;
    const unsigned inside = left >= ROWS ? FULL : (1u << left) - 1;
    return (unsigned)uniform_of((int)(word & inside));
  };
  auto first_tile = [](unsigned avail) -> int { return TILES == 2 && !(avail & 0xffffu) ? 1 : 0; };      // avail != 0
  auto load = [&](long long w, int h, int chunk, unsigned avail, f16x8 (&ga)[NKS]) {
    many_load_frags<NKS>(gallery, d, TILES * w + h, chunk, TILES == 1 ? avail : (avail >> (16 * h)) & 0xffffu, u, kq, ga);
  };

  f16x8 fa[NKS], fb[NKS];
  long long wc = blockIdx.x;
  unsigned ac = avail_at(wc, word_at(wc));
  while (wc < n_units && !ac) {
    dead(wc);
    wc += G;
    ac = avail_at(wc, word_at(wc));
  }
  if (wc >= n_units) return;                               // uniform for the workgroup
  unsigned w1 = word_at(wc + G);
  int hc = first_tile(ac), chunk = 0;
  load(wc, hc, 0, ac, fa);
  auto step = [&](const f16x8 (&cur)[NKS], f16x8 (&nxt)[NKS]) -> bool {
    long long wn = wc;
    unsigned an = ac;
    int hn = hc, cn = chunk + 1;
    if (cn == nchunks) {
      cn = 0;
      if (TILES == 2 && hc == 0 && (ac >> 16)) {
        hn = 1;                                            // the unit's second tile
      } else {
        wn = wc + G;
        an = avail_at(wn, w1);
        while (wn < n_units && !an) {
          dead(wn);
          wn += G;
          an = avail_at(wn, word_at(wn));
        }
        w1 = word_at(wn + G);
        hn = first_tile(an);
      }
    }
    const bool last = wn >= n_units;
    if (last) load(wc, hc, chunk, ac, nxt);
    else load(wn, hn, cn, an, nxt);
    compute(wc, hc, ac, chunk, cur);
    wc = wn, ac = an, hc = hn, chunk = cn;
    return !last;
  };
  while (step(fa, fb) && step(fb, fa)) {
  }
}

// ---- the host side of a pass
// workgroups a CU holds: a workgroup of g waves keeps g x 32 KB of B fragments in the LDS (and the search 8 KB of lists a wave: 160 KiB
// a CU), so 4 / g fit; four one-wave workgroups already give every SIMD a wave
inline int many_per_cu(int nq) {
  const int g = many_qgroups(nq);
  return g == 1 ? 4 : (g == 2 ? 2 : 1);
}
// dynamic LDS of the call's images (ManyImage), of all its waves: at most 128 KiB
inline size_t many_img_lds_bytes(int nq, int d) { return (size_t)many_qgroups(nq) * many_img_vecs(d, many_item_steps(d)) * sizeof(uint4); }
// f(MASKED, NKS as integral constants) for the pass of a call: MASKED by `live`, NKS = many_item_steps(d)
template <typename F>
int many_with_pass(bool masked, int d, F f) {
  auto of = [&](auto m) -> int {
    const int nks = many_item_steps(d);
    if (nks == 16) return f(m, std::integral_constant<int, 16>{});
    if (nks == 8) return f(m, std::integral_constant<int, 8>{});
    if (nks == 4) return f(m, std::integral_constant<int, 4>{});
    return f(m, std::integral_constant<int, 2>{});
  };
  return masked ? of(std::true_type{}) : of(std::false_type{});
}
}  // namespace
