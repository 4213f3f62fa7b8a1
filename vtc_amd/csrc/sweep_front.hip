// sweep_front.hip -- what the retrieval sweeps share before they diverge (declared in sweep_common.h): the row norms and the split-bf16
// operand rows of the distance-matrix sweeps, the fused prologue and the workspace of the block-minima sweeps, the blocking of a row pass,
// the two error constants, and the C ABI's k list.  sweep_topk.hip, sweep_recall.hip and sweep_rank.hip start from here.
#include "sweep_common.h"

#include <algorithm>

using namespace vtcsweep;

namespace {

__global__ __launch_bounds__(256) void row_sqnorm_kernel(const float *__restrict__ x, float *__restrict__ out, int n, int d) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const float *xr = x + (size_t)r * d;
  float s = 0.f;
  for (int c = lane; c < d; c += 64) s += xr[c] * xr[c];
  s = wave_sum(s);
  if (lane == 0) out[r] = s;
}

// out[r] = [hi | lo | hi] (query side, side = 0) or [hi | hi | lo] (gallery side, side = 1); parts = 1 => [hi]
__global__ __launch_bounds__(256) void split_bf16_kernel(const float *__restrict__ x, bf16_t *__restrict__ out, int n, int d,
                                                         int parts, int side) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n * d) return;
  const size_t r = i / d;
  const int c = (int)(i - r * d);
  const float v = x[i];
  const bf16_t hi = f2bf(v);
  bf16_t *o = out + r * (size_t)(parts * d);
  o[c] = hi;
  if (parts == 3) {
    const bf16_t lo = f2bf(v - bf2f(hi));
    o[d + c] = side == 0 ? lo : hi;
    o[2 * d + c] = side == 0 ? hi : lo;
  }
}

// ---- fused prologue of the block-minima sweep (round 4): one launch for BOTH embedding sets ---------------------------------
// Per row x (one wave): |x|^2 (fp32), the bf16 operand row x~ = rne(x) (xb == NULL: statistics only), and the two numbers the
// certificate's error bound is made of -- |x~| and |e| with e = x - x~, the row's ACTUAL rounding error (exact in fp32: x and x~
// agree in sign, exponent and the top mantissa bits, so the difference is representable) -- plus the running maxima of all three
// over the set (per-block maxima, folded by sweep_prep_max_kernel).
//   | q~.g~ - q.g | = | q~.e_g + e_q.g~ + e_q.e_g |  <=  |q~||e_g| + |e_q||g~| + |e_q||e_g|          (Cauchy-Schwarz)
// With |e| <= 2^-8 |x| this is the worst-case bound of rounds 2-3 (2u + u^2)|q||g|; on real embeddings |e| ~ 0.4 x 2^-8 |x|, so
// the bound is ~0.45 x that and the candidate sets shrink accordingly -- and rows that do sit on bf16 midpoints (the adversarial test) still get the
// full bound, because |e| is measured, not assumed.  Both norms carry a 1e-4 relative slack for their fp32 summation.
struct PrepSide {
  const float *x;
  bf16_t *xb;
  float *n2;
  float2 *st;      // (|x~|, |e|) per row
  float *mx;       // [0] max |x|^2, [1] max |x~|, [2] max |e|   (written by sweep_prep_max_kernel)
  int n;
};
constexpr int PREP_RPW = 4;      // rows per wave
// part[block][8]: the block's maxima {A: |x|^2, |x~|, |e|, -; B: ...} -- no atomics (20 000 rows x 3 atomic maxima on two sets of
// three words took 0.5 ms); sweep_prep_max_kernel folds the blocks' rows
__global__ __launch_bounds__(256) void sweep_prep_kernel(PrepSide A, PrepSide B, int d, float *__restrict__ part) {
  __shared__ float red[4][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float mx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < PREP_RPW; ++i) {
    int r = (blockIdx.x * 4 + wave) * PREP_RPW + i;
    if (r >= A.n + B.n) break;                   // wave-uniform
    const bool second = r >= A.n;
    const PrepSide &S = second ? B : A;
    if (second) r -= A.n;
    const float *xr = S.x + (size_t)r * d;
    float n2 = 0.f, nt2 = 0.f, e2 = 0.f;
    for (int c = lane * 4; c < d; c += 256) {
      const float4 v = *reinterpret_cast<const float4 *>(xr + c);
      const float f[4] = {v.x, v.y, v.z, v.w};
      unsigned short h[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        h[j] = f2bf(f[j]);
        const float t = bf2f(h[j]), e = f[j] - t;
        n2 = fmaf(f[j], f[j], n2);
        nt2 = fmaf(t, t, nt2);
        e2 = fmaf(e, e, e2);
      }
      if (S.xb) *reinterpret_cast<uint2 *>(S.xb + (size_t)r * d + c) = make_uint2((unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16));
    }
    n2 = wave_sum(n2); nt2 = wave_sum(nt2); e2 = wave_sum(e2);
    // (+ d x FLT_MIN under the roots: a component below ~1e-19 squares to a flushed zero, and up to d such terms may be missing from
    //  either sum -- ADVICE r4; on unit-norm rows the addend is 6e-36 beside 1e-6 .. 1 and changes no bit)
    const float nt = sqrtf(nt2 + (float)d * 1.1754944e-38f) * 1.0001f, e = sqrtf(e2 + (float)d * 1.1754944e-38f) * 1.0001f;
    if (lane == 0) {
      S.n2[r] = n2;
      S.st[r] = make_float2(nt, e);
    }
    const int o = second ? 4 : 0;
    mx[o] = fmaxf(mx[o], n2); mx[o + 1] = fmaxf(mx[o + 1], nt); mx[o + 2] = fmaxf(mx[o + 2], e);
  }
  if (lane < 8) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) v = lane == k ? mx[k] : v;
    red[wave][lane] = v;
  }
  __syncthreads();
  if (threadIdx.x < 8) part[(size_t)blockIdx.x * 8 + threadIdx.x] = fmaxf(fmaxf(red[0][threadIdx.x], red[1][threadIdx.x]), fmaxf(red[2][threadIdx.x], red[3][threadIdx.x]));
}
__global__ __launch_bounds__(256) void sweep_prep_max_kernel(const float *__restrict__ part, int nblocks, float *__restrict__ mxA, float *__restrict__ mxB,
                                                             int *zero_a, int *zero_b) {
  __shared__ float red[32][8];
  if (threadIdx.x == 0) {          // (the recall-rank path's two fallback counters: saves a fill launch)
    if (zero_a) *zero_a = 0;
    if (zero_b) *zero_b = 0;
  }
  const int k = threadIdx.x & 7, sl = threadIdx.x >> 3;
  float m = 0.f;
  for (int b = sl; b < nblocks; b += 32) m = fmaxf(m, part[(size_t)b * 8 + k]);
  red[sl][k] = m;
  __syncthreads();
  if (threadIdx.x < 8) {
    float v = 0.f;
    for (int i = 0; i < 32; ++i) v = fmaxf(v, red[i][threadIdx.x]);
    if (threadIdx.x < 3) mxA[threadIdx.x] = v;
    else if (threadIdx.x >= 4 && threadIdx.x < 7) mxB[threadIdx.x - 4] = v;
  }
}
static int prep_blocks(int rows) { return cdiv(rows, 4 * PREP_RPW); }
static void launch_sweep_prep(const PrepSide &A, const PrepSide &B, int d, float *part, hipStream_t stream, int *zero_a = nullptr, int *zero_b = nullptr) {
  const int nb = prep_blocks(A.n + B.n);
  hipLaunchKernelGGL(sweep_prep_kernel, dim3(nb), dim3(256), 0, stream, A, B, d, part);
  hipLaunchKernelGGL(sweep_prep_max_kernel, dim3(1), dim3(256), 0, stream, part, nb, A.mx, B.mx, zero_a, zero_b);
}
}  // namespace

namespace vtcsweep {

void launch_norms_split(const float *queries, int nq, float *qn, bf16_t *qb, const float *gallery, int ng, float *gn, bf16_t *gb, int d, int parts,
                        hipStream_t stream, int q0, int q_rows) {
  hipLaunchKernelGGL(row_sqnorm_kernel, dim3(cdiv(nq, 4)), dim3(256), 0, stream, queries, qn, nq, d);
  hipLaunchKernelGGL(row_sqnorm_kernel, dim3(cdiv(ng, 4)), dim3(256), 0, stream, gallery, gn, ng, d);
  if (parts == 0) return;
  if (q_rows < 0) q0 = 0, q_rows = nq;
  if (q_rows > 0)
    hipLaunchKernelGGL(split_bf16_kernel, dim3((unsigned)(((size_t)q_rows * d + 255) / 256)), dim3(256), 0, stream, queries + (size_t)q0 * d, qb, q_rows, d,
                       parts, 0);
  hipLaunchKernelGGL(split_bf16_kernel, dim3((unsigned)(((size_t)ng * d + 255) / 256)), dim3(256), 0, stream, gallery, gb, ng, d, parts, 1);
}

// rows_per_block = 0: as many rows of `cols` fp32 distances as fit a 2 GiB block, a multiple of 256.
// Big blocks: a block's top-k pass costs one list warm-up per (row, segment) wave, and the GEMM a fill/drain
// per launch, so FEWER, LARGER blocks win over Infinity-Cache residency (measured at 50k x 50k, F32 /
// BF16X3, one direction: 128 MiB blocks 27.5 / 19.6 ms, 2 GiB blocks 21.4 / 10.4 ms; top-k 1.5 -> 5.0 TB/s).
int default_rows_per_block(int cols) {
  const size_t budget = (size_t)2 << 30;
  const int rpb = (int)std::min<size_t>(budget / ((size_t)cols * 4), (size_t)1 << 20) / 256 * 256;
  return rpb < 256 ? 256 : rpb;
}

// A row pass over a [rows, cols] block: enough (row, segment) waves to fill the chip (32 waves per CU), in segments of whole 1024-column
// steps (every segment pays its own warm-up insertions, so segments are used only when rows alone cannot fill the chip).
RowSegments row_segments(int rows, int cols) {
  const int S = std::min(MAX_SEG, cdiv(8192, rows));
  const int seg_cols = cdiv(cdiv(cols, S), 1024) * 1024;
  return {cdiv(cols, seg_cols), seg_cols};
}

// worst-case error of a split-bf16 (BF16X3) distance, relative to |q|^2 + max|g|^2: what certifies the distance-matrix path's candidate lists
// (sweep_topk.hip, exact_finish_lists) and sets the full-rank sweep's thresholds (sweep_rank.hip; vtc_l2_rank_kappa reports it).
// With u = 2^-8 (bf16's unit roundoff): x = hi + lo + r, |lo| <= u |x|, |r| <= u^2 |x|; the GEMM forms hi.hi + hi.lo + lo.hi,
// so the product misses lo.lo (u^2 |q||g|) and the two residual terms (2 u^2 |q||g|): 3 u^2 |q||g| <= 3 u^2 (|q|^2 + |g|^2) / 2,
// twice that on the distance = 3 * 2^-16 (rounds 1-2 had 3 * 2^-18); fp32 accumulation of 3 d products (3 d * 2^-24), fp32 row
// norms (d * 2^-24), the epilogue's three roundings.
float split_kappa(int d) { return 3.0f / 65536.0f + 4.0f * d / 16777216.0f + 1e-6f; }

// The block-minima path's constant: worst-case |approx - exact| of a plain-bf16 key's distance, relative to |q|^2 + max|g|^2.  bf16 keeps 8 significant bits, so its unit
// roundoff under round-to-nearest-even is u = 2^-8 (NOT 2^-9: rounds 1-2 had half this constant -- random embeddings sit far
// inside either bound, coordinated roundings on bf16 midpoints do not: tests/test_gpu_sweep.py adversarial case):
//   q~.g~ - q.g = sum q e_g + g e_q + e_q e_g,  |e| <= u |x|   =>   |.| <= (2u + u^2) |q||g| <= (2u + u^2)(|q|^2 + |g|^2) / 2,
// twice that on the distance: 2^-7 (1 + 2^-9); fp32 accumulation of d products and the two fp32 norms (2 d 2^-24); the 7 index
// bits of the key (2^-16 of a distance <= 2 (|q|^2 + |g|^2)); the epilogue's roundings (slack)
// (round 4: the operand-rounding term is no longer this worst case but the rows' measured |e| -- sweep_prep_kernel / minsel_kernel;
// what remains here are the fp32 terms, relative to |q|^2 + max|g|^2)
bool exact2_enabled(int ng, int nq, int depth) { return depth <= 32 && ng >= 1024 && nq >= 1; }
float exact2_kappa(int d) { return 2.0f * d / 16777216.0f + 1.0f / 32768.0f + 1e-6f; }

Sweep2Ws plan2(char *ws, int ng, int nq, int d, bool bidir) {
  Sweep2Ws s;
  Bump b(ws);
  auto take = [&](size_t bytes) { return b.take(bytes); };
  s.nblk_c = cdiv(ng, 64);
  s.nblk_r = cdiv(nq, RB2);
  s.qn = (float *)take((size_t)nq * 4);
  s.gn = (float *)take((size_t)ng * 4);
  s.gmax = (float *)take(256);
  s.qmax = (float *)take(256);
  s.qst = (float2 *)take((size_t)nq * 8);
  s.gst = (float2 *)take((size_t)ng * 8);
  s.pmax = (float *)take((size_t)((nq + ng) / 16 + 2) * 8 * 4);
  s.qb = (bf16_t *)take((size_t)nq * d * 2);
  s.gb = (bf16_t *)take((size_t)ng * d * 2);
  s.rowk = (unsigned *)take((size_t)L2MIN_PLANES * s.nblk_c * nq * 4);
  s.colk = bidir ? (unsigned *)take((size_t)L2MIN_PLANES * s.nblk_r * ng * 4) : nullptr;
  s.cand = (int64_t *)take((size_t)nq * CD2 * 8);
  s.cand_n = (int *)take((size_t)nq * 4);
  s.theta = (float *)take((size_t)nq * 4);
  s.cand2 = nullptr; s.cand2_n = nullptr; s.theta2 = nullptr;
  if (bidir) {
    s.cand2 = (int64_t *)take((size_t)ng * CD2 * 8);
    s.cand2_n = (int *)take((size_t)ng * 4);
    s.theta2 = (float *)take((size_t)ng * 4);
  }
  s.flags = (int *)take((size_t)(std::max(nq, bidir ? ng : 0) + 1) * 4);
  s.flags2 = bidir ? (int *)take((size_t)(ng + 1) * 4) : nullptr;
  s.total = b.off;
  return s;
}

// Prologue of every block-minima entry point: norms, rounding-error statistics and their maxima of both sets in ONE launch (rounds 1-3:
// six), which also zeroes up to two fallback counters.  round_operands: the bf16 operand rows too (false: statistics only -- the
// operands were rounded by the ranks that ran the GEMMs, with this same rounding).
void sweep_prologue(const Sweep2Ws &s, const float *queries, int nq, const float *gallery, int ng, int d, bool round_operands,
                    hipStream_t stream, int *zero_a, int *zero_b) {
  ProfScope prof(VTC_PROF_TOPK, (double)(nq + ng) * d * (round_operands ? 6 : 4), stream);
  const PrepSide A{queries, round_operands ? s.qb : nullptr, s.qn, s.qst, s.qmax, nq}, B{gallery, round_operands ? s.gb : nullptr, s.gn, s.gst, s.gmax, ng};
  launch_sweep_prep(A, B, d, s.pmax, stream, zero_a, zero_b);
}

// Sharded sweep: the column planes go to a [npl, nblk_pad, n_cols] buffer sized for the LARGEST shard; the row blocks this rank has no
// rows for (shards differ by a row) hold +inf keys.
void fill_absent_row_blocks(unsigned *colk, int npl, int nblk_pad, int nblk, int n_cols, hipStream_t stream) {
  for (int pl = 0; pl < npl && nblk_pad > nblk; ++pl)
    (void)hipMemsetD32Async((hipDeviceptr_t)(colk + ((size_t)pl * nblk_pad + nblk) * n_cols), VTC_L2MIN_INF, (size_t)(nblk_pad - nblk) * n_cols, stream);
}

int read_k(KList &kl, const char *fn, const int *k_vals, int nk, int k_limit) {
  VTC_CHECK(k_vals && nk >= 1 && nk <= 4, "%s: nk=%d must be in [1, 4]", fn, nk);
  kl = KList{{0, 0, 0, 0}, nk, 0};
  for (int i = 0; i < nk; ++i) {
    VTC_CHECK(k_vals[i] >= 1 && k_vals[i] <= k_limit, "%s: k=%d outside [1, %d]", fn, k_vals[i], k_limit);
    kl.k[i] = k_vals[i];
    kl.kmax = std::max(kl.kmax, k_vals[i]);
  }
  return 0;
}

}  // namespace vtcsweep

// rows per column block of the sharded sweeps' exchanged key planes (include/vtc_hip.h)
extern "C" int vtc_l2_sweep_row_block(void) { return RB2; }
