// sweep_rank.hip -- the full-rank sweep: the exact rank of EVERY pair's target (median / mean rank, MRR, recall at any k) by COUNTING over
// the blocks of one BF16X3 distance matrix, fp64 for the entries within the error bound of a target.
//   vtc_l2_rank_bidir           both directions of n paired rows
//   vtc_l2_rank_shard           the same sweep over a window of the rows: one rank's share of a row-sharded evaluation, partial column counts
//   vtc_l2_rank_grouped         videos with several captions each: the sweep made rectangular, the target taken from a table
//   vtc_l2_rank_grouped_vunit   that sweep with a third direction: video -> text counted in VIDEOS (groups of captions), not captions
// Norms, operand split, blocking and the error constant are sweep_front.hip's; the fp64 distance is sweep_common.h's.
#include "sweep_common.h"

#include <algorithm>
#include <type_traits>

using namespace vtcsweep;

namespace {

// ---- full-rank sweep (vtc_l2_rank_bidir): COUNT instead of select ------------------------------------------------------------------
// rank_i = #{ j : (|q_i - g_j|^2, j) < (|q_i - g_t|^2, t) } for EVERY query, wherever its target landed (median / mean rank, MRR, recall at
// any k), in both directions of n paired rows from the blocks of ONE split-bf16 distance matrix D[i][j] ~ |b_i - a_j|^2 (the BF16X3 GEMM of
// sweep_topk.hip).  With d_t the target's fp64 distance and eps = split_kappa (|q|^2 + max|g|^2) the bound that certifies the BF16X3 lists
// there, an entry v of the query's row (gallery a) or column (gallery b) is
//   v < lo = rd(d_t - eps)   closer for certain: counted;     v > hi = ru(d_t + eps)   farther for certain: dropped;
//   else (a NaN entry too)   in reach: the pair (owner, other) goes to the direction's reach pool and fp64 decides (rank_settle_kernel).
// An owner whose pairs did not fit the pool is flagged and counted again by fp64 brute force over the whole other side
// (rank_brute_kernel), so the ranks do not depend on the pool's capacity.  A pair whose target distance is not finite gets rank n.
constexpr int RS_STATS = 8;           // 64-bit words at the head of the workspace (include/vtc_hip.h, vtc_l2_rank_bidir)
constexpr int RS_STATS_V = 8;         // behind them, the video-unit direction's (vtc_l2_rank_grouped_vunit): three figures, five unused words
constexpr int RS_NB = 8;              // fp64 distances a wave forms at once

// max of the FINITE squared norms of each side (a non-finite row's entries are NaN / inf whatever the bound says; with it in the maximum
// every query of the direction would have the whole gallery in reach)
__global__ __launch_bounds__(256) void rank_max_kernel(const float *__restrict__ xa, int na, const float *__restrict__ xb, int nb,
                                                       float *__restrict__ out_a, float *__restrict__ out_b) {
  __shared__ float part[4];
  const float *x = blockIdx.x ? xb : xa;
  const int n = blockIdx.x ? nb : na;
  float m = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float v = x[i];
    m = v < INFINITY ? fmaxf(m, v) : m;
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) *(blockIdx.x ? out_b : out_a) = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

// per-direction state of the counting sweep
struct RankDir {
  const float *own, *other;      // [n_own, d], [n_other, d] fp32: the direction's queries and its gallery
  const float *lo, *hi;          // [n_own] thresholds of the owner's row / column of D (hi = -inf: the owner's target distance is not finite)
  int *cnt;                      // [n_own] entries closer than the target
  int *reach;                    // [n_own] entries in reach of the target (statistics)
  int *ovf;                      // [n_own] != 0: the owner's pairs did not fit the pool
  int2 *pool;                    // [cap] (owner, other)
  unsigned long long *pool_n;    // pairs offered to the pool (may exceed cap)
  unsigned long long cap;
  const double *dt;              // [n_own] fp64 distance of the owner to its target (paired: one array for both directions)
  int n_own, n_other;
  int tgt0;                      // paired: owner o's target is tgt0 + o.  The row direction of a row window (vtc_l2_rank_shard) numbers its owners
                                 // from the window's first row, so tgt0 = that row; 0 everywhere else.  `own` starts at the direction's owner 0.
};
// The kernels below take the direction as a compile-time policy that says ONE thing, where an owner's target is: its own index (RankDir,
// vtc_l2_rank_bidir) or an entry of a table (RankDirG, vtc_l2_rank_grouped).
struct RankDirG : RankDir {
  const int *tgt;                // [n_own] the owner's target on the other side (-1: none, and hi = -inf)
};
template <typename Dir> constexpr bool rank_has_table = std::is_same<Dir, RankDirG>::value;
template <typename Dir>
__device__ __forceinline__ int rank_target(const Dir &P, int owner) {
  if constexpr (rank_has_table<Dir>) return P.tgt[owner];
  else return P.tgt0 + owner;
}

// What the prologue writes for a direction: the owners' target distances and thresholds, from their norms and the other side's maximum.
struct RankThresholds {
  const float *n2, *other_max;   // [n_own] |q|^2; max |g|^2 over the finite rows of the other side
  double *dt;
  float *lo, *hi;
};
__device__ __forceinline__ void rank_set_thresholds(const RankThresholds &T, int i, double dt, float kappa) {
  const bool ok = dt < (double)INFINITY;                // false for NaN too
  const float eps = kappa * (T.n2[i] + *T.other_max);
  T.lo[i] = ok ? __double2float_rd(dt - (double)eps) : -INFINITY;
  T.hi[i] = ok ? __double2float_ru(dt + (double)eps) : -INFINITY;
}

// One wave per 8 rows of D, ALL n_rows of them (`rows`: their queries, b): the fp64 distance of the row to its target, the counters' zeroes,
// and the row direction's thresholds for the rows it owns -- TR is indexed by the direction's owner, row - R.tgt0 (every row but in a row
// window).  Paired: the column direction's owner i has the same target distance, so its thresholds are written here too, for every i
// whatever the window (TC.dt is the whole array, TR.dt the same array from the window's first row), and the columns [n, n_ld) that pad
// the matrix's rows to 16 bytes get lo = hi = -inf: the column pass neither counts nor pools them.  Grouped:
// rank_grouped_target_kernel writes the column direction (TC is not read).
template <typename Dir>
__global__ __launch_bounds__(256) void rank_prep_kernel(const Dir R, const float *__restrict__ rows, int n_rows, const RankThresholds TR,
                                                        const RankThresholds TC, int n_ld, int d, float kappa, int *__restrict__ zero, int n_zero) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  for (int i = t; i < n_zero; i += gridDim.x * 256) zero[i] = 0;
  if constexpr (!rank_has_table<Dir>) {
    const int n = R.n_other;
    if (t < n_ld - n) TC.lo[n + t] = TC.hi[n + t] = -INFINITY;
  }
  const int lane = threadIdx.x & 63;
  const int i0 = (t >> 6) * RS_NB;
  if (i0 >= n_rows) return;                             // wave-uniform
  int qi[RS_NB], gi[RS_NB];
#pragma unroll
  for (int u = 0; u < RS_NB; ++u) {
    qi[u] = min(i0 + u, n_rows - 1);
    if constexpr (rank_has_table<Dir>) gi[u] = R.tgt[qi[u]];
    else gi[u] = qi[u];
  }
  double dd[RS_NB];
  wave_dist64_pairs(rows, R.other, qi, gi, d, lane, dd);
  double mine = 0.0;
#pragma unroll
  for (int u = 0; u < RS_NB; ++u) mine = lane == u ? dd[u] : mine;
  const int i = i0 + lane;
  if (lane < RS_NB && i < n_rows) {
    const int o = i - R.tgt0;
    if (o >= 0 && o < R.n_own) {
      TR.dt[o] = mine;
      rank_set_thresholds(TR, o, mine, kappa);          // rows of D: query b_i against the a's
    }
    if constexpr (!rank_has_table<Dir>) {
      TC.dt[i] = mine;
      rank_set_thresholds(TC, i, mine, kappa);          // columns: query a_i against the b's
    }
  }
}

// inclusive prefix sum of x over the wave's lanes
__device__ __forceinline__ int wave_incl_scan(int x, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(x, o, 64);
    x += lane >= o ? up : 0;
  }
  return x;
}

// Wave-wide append of the lanes' in-reach pairs: `m` has a bit per candidate slot of the lane, other(q) its index on the other side,
// owner(q) its owner.  ONE atomic per wave reserves the room; a pair past the capacity flags its owner instead.
template <int NSLOT, typename OwnerFn, typename OtherFn>
__device__ __forceinline__ void rank_pool_append(const RankDir &P, unsigned m, int lane, OwnerFn owner, OtherFn other) {
  const int nr = __popc(m);
  const int incl = wave_incl_scan(nr, lane);
  const int total = __shfl(incl, 63, 64);
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(P.pool_n, (unsigned long long)total);
  base = __shfl(base, 0, 64);
  unsigned long long pos = base + (unsigned long long)(incl - nr);
#pragma unroll
  for (int q = 0; q < NSLOT; ++q) {
    if ((m >> q) & 1u) {
      if (pos < P.cap) P.pool[pos] = make_int2(owner(q), other(q));
      else P.ovf[owner(q)] = 1;
      ++pos;
    }
  }
}

// The same through a wave-private staging buffer in LDS (RS_STAGE pairs): the atomic that reserves room in the pool returns a value the wave
// has to wait for, and with a pair or two in reach in most steps of a scan that wait was the scan (10k: 0.34 of the row pass's ms).  Staged,
// a wave pays it once per RS_STAGE pairs and once at its end (rank_stage_flush).  A step with more pairs than the buffer holds goes direct.
constexpr int RS_STAGE = 256;
__device__ __forceinline__ void rank_stage_flush(const RankDir &P, const int2 *stage, int &n_st, int lane) {
  if (n_st == 0) return;                                   // wave-uniform
  __builtin_amdgcn_wave_barrier();
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(P.pool_n, (unsigned long long)n_st);
  base = __shfl(base, 0, 64);
  for (int i = lane; i < n_st; i += 64) {
    const int2 e = stage[i];
    if (base + (unsigned long long)i < P.cap) P.pool[base + (unsigned long long)i] = e;
    else P.ovf[e.x] = 1;
  }
  __builtin_amdgcn_wave_barrier();
  n_st = 0;
}
template <int NSLOT, typename OwnerFn, typename OtherFn>
__device__ __forceinline__ void rank_stage_append(const RankDir &P, int2 *stage, int &n_st, unsigned m, int lane, OwnerFn owner, OtherFn other) {
  const int nr = __popc(m);
  const int incl = wave_incl_scan(nr, lane);
  const int total = __shfl(incl, 63, 64);
  if (n_st + total > RS_STAGE) rank_stage_flush(P, stage, n_st, lane);       // wave-uniform
  if (total > RS_STAGE) {                                                    // wave-uniform: a dense step (duplicates, clusters)
    rank_pool_append<NSLOT>(P, m, lane, owner, other);
    return;
  }
  int pos = n_st + incl - nr;
#pragma unroll
  for (int q = 0; q < NSLOT; ++q) {
    if ((m >> q) & 1u) stage[pos++] = make_int2(owner(q), other(q));
  }
  n_st += total;
}

// Row direction: one wave per (row of the block, column segment), streaming as row_topk_kernel does (1024 columns per step, four 16-byte
// loads per lane, two steps in flight behind the one being counted; the last columns of a row whose n_cols is no multiple of four are loaded
// one by one).  Per value two compares; one atomic per wave at the end.
template <typename Dir>
__global__ __launch_bounds__(256) void rank_row_count_kernel(const float *__restrict__ dist, int ld, int n_rows, int n_cols, int row0, int S,
                                                             int seg_cols, const Dir P) {
  __shared__ int2 stage_all[4][RS_STAGE];
  const int lane = threadIdx.x & 63;
  int2 *stage = stage_all[threadIdx.x >> 6];              // wave-private
  int n_st = 0;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n_rows * S) return;
  const int r = w / S, seg = w - r * S;
  const int gr = row0 + r;                                // the owner
  const float lo = P.lo[gr], hi = P.hi[gr];
  if (hi == -INFINITY) return;                            // wave-uniform: target distance not finite, rank n
  const int tg = rank_target(P, gr);                      // the column of its target
  const float *row = dist + (size_t)r * ld;               // (ld % 4 == 0: 16-byte aligned at every multiple of four columns)
  const int c_lo = seg * seg_cols, c_hi = min(n_cols, c_lo + seg_cols);
  auto load_step = [&](int base, float (&v)[16]) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int c = base + 256 * h + lane * 4;
      if (c + 3 < c_hi) {
        typedef float v4f_t __attribute__((ext_vector_type(4)));
        const v4f_t t = __builtin_nontemporal_load(reinterpret_cast<const v4f_t *>(row + c));
        v[4 * h] = t.x; v[4 * h + 1] = t.y; v[4 * h + 2] = t.z; v[4 * h + 3] = t.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * h + e] = c + e < c_hi ? row[c + e] : INFINITY;
      }
    }
  };
  float cur[16], nxt[16], nx2[16];
  load_step(c_lo, cur);
  if (c_lo + 1024 < c_hi) load_step(c_lo + 1024, nxt);
  int closer = 0, n_reach = 0;
  for (int base = c_lo; base < c_hi; base += 1024) {
    if (base + 2048 < c_hi) load_step(base + 2048, nx2);
    unsigned m = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int idx = base + 256 * (q >> 2) + lane * 4 + (q & 3);
      const bool ok = idx < c_hi && idx != tg;
      const bool lt = cur[q] < lo;
      closer += (ok && lt) ? 1 : 0;
      m |= (ok && !lt && !(cur[q] > hi)) ? (1u << q) : 0u;
    }
    if (__ballot(m != 0) != 0ull) {                       // wave-uniform, rare: entries within eps of the target's distance
      n_reach += __popc(m);
      rank_stage_append<16>(P, stage, n_st, m, lane, [&](int) { return gr; }, [&](int q) { return base + 256 * (q >> 2) + lane * 4 + (q & 3); });
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) { cur[q] = nxt[q]; nxt[q] = nx2[q]; }
  }
  rank_stage_flush(P, stage, n_st, lane);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { closer += __shfl_xor(closer, o, 64); n_reach += __shfl_xor(n_reach, o, 64); }
  if (lane == 0) {
    if (closer) atomicAdd(&P.cnt[gr], closer);
    if (n_reach) atomicAdd(&P.reach[gr], n_reach);
  }
}

// What the two column passes (rank_col_count_kernel, rank_vunit_count_kernel) share.  A lane owns four adjacent columns c .. c + 3 and is
// one of four row sub-lanes (lane >> 4) of its columns.  Preamble: the columns' thresholds and zeroed counters; -inf for a lane past the
// matrix, a padding column, or an owner whose target distance is not finite.
constexpr int RS_V = 4;
__device__ __forceinline__ void rank_col_thresholds(const RankDir &P, int c, bool live, float (&lo)[RS_V], float (&hi)[RS_V], int (&cnt)[RS_V],
                                                    int (&reach)[RS_V]) {
#pragma unroll
  for (int e = 0; e < RS_V; ++e) {
    lo[e] = live ? P.lo[c + e] : -INFINITY;
    hi[e] = live ? P.hi[c + e] : -INFINITY;
    cnt[e] = 0; reach[e] = 0;
  }
}
// Tail: the lanes' counts folded over the four row sub-lanes, one atomic per column and wave.
__device__ __forceinline__ void rank_col_commit(const RankDir &P, int c, bool live, int sub, int (&cnt)[RS_V], int (&reach)[RS_V]) {
#pragma unroll
  for (int e = 0; e < RS_V; ++e) {
    cnt[e] += __shfl_xor(cnt[e], 16, 64); cnt[e] += __shfl_xor(cnt[e], 32, 64);
    reach[e] += __shfl_xor(reach[e], 16, 64); reach[e] += __shfl_xor(reach[e], 32, 64);
    if (live && sub == 0) {
      if (cnt[e]) atomicAdd(&P.cnt[c + e], cnt[e]);
      if (reach[e]) atomicAdd(&P.reach[c + e], reach[e]);
    }
  }
}

// Column direction of the same block: one wave per (strip of 64 columns, row segment).  The rows are 16-byte aligned (ld % 4 == 0 and
// n_cols = ld: the padding columns are scanned, their hi = -inf): a lane owns four adjacent columns and every fourth row -- a load
// instruction of the wave is four 256-byte row pieces.  Eight loads per lane in flight; the lanes' counts are folded over the wave once,
// behind the scan: one atomic per column and wave.  The counts are CARRIED from one block of rows to the next in P.cnt (global row ids:
// row_id0 + row).
template <typename Dir>
__global__ __launch_bounds__(256) void rank_col_count_kernel(const float *__restrict__ dist, int ld, int n_rows, int n_cols, int row_id0,
                                                             int n_strips, int S, int seg_rows, const Dir P) {
  constexpr int U = 8, V = RS_V;                          // loads in flight per lane; columns per lane = rows per load instruction of the wave
  __shared__ int2 stage_all[4][RS_STAGE];
  int2 *stage = stage_all[threadIdx.x >> 6];              // wave-private
  int n_st = 0;
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n_strips * S) return;
  const int seg = w / n_strips, strip = w - seg * n_strips;   // neighbouring waves: neighbouring strips of the same rows
  const int c_strip = strip * 64 + 4 * (lane & 15);
  const bool live = c_strip < n_cols;                     // (n_cols % 4 == 0: the lane's four columns are in or out together)
  const int c = live ? c_strip : 0;                       // a lane past the matrix reads column 0 and counts nothing
  const int sub = lane >> 4;
  const int r_lo = seg * seg_rows, r_hi = min(n_rows, r_lo + seg_rows);
  float lo[V], hi[V];
  int cnt[V], reach[V], tg[V];                            // tg: the row (global id) of the column's target
  rank_col_thresholds(P, c, live, lo, hi, cnt, reach);
  // Table form: tgt has n_cols >= 4 entries, the padding ones written too; a lane past it reads tgt[0 .. 3].  Paired: a column's target is
  // the row of its own number in every row window -- written out, not rank_target(): the column direction's tgt0 is always 0, and reading
  // it costs this instantiation four VGPRs and the fifth wave per SIMD (profiles/rank_shard.md).
#pragma unroll
  for (int e = 0; e < V; ++e) {
    if constexpr (rank_has_table<Dir>) tg[e] = P.tgt[c + e];
    else tg[e] = c + e;
  }
  for (int rb = r_lo; rb < r_hi; rb += V * U) {
    float v[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = rb + u * V + sub;
      const float4 t = *reinterpret_cast<const float4 *>(dist + (size_t)min(row, r_hi - 1) * ld + c);      // branch-free: all loads of a lane in flight together
      v[u][0] = t.x; v[u][1] = t.y; v[u][2] = t.z; v[u][3] = t.w;
    }
    unsigned m = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = rb + u * V + sub;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const bool ok = row < r_hi && hi[e] != -INFINITY && row_id0 + row != tg[e];
        const bool lt = v[u][e] < lo[e];
        cnt[e] += (ok && lt) ? 1 : 0;
        const bool in = ok && !lt && !(v[u][e] > hi[e]);
        reach[e] += in ? 1 : 0;
        m |= in ? (1u << (u * V + e)) : 0u;
      }
    }
    if (__ballot(m != 0) != 0ull)                          // wave-uniform, rare
      rank_stage_append<U * V>(P, stage, n_st, m, lane, [&](int q) { return c + q % V; }, [&](int q) { return row_id0 + rb + (q / V) * V + sub; });
  }
  rank_stage_flush(P, stage, n_st, lane);
  rank_col_commit(P, c, live, sub, cnt, reach);
}

// The pooled pairs of both directions, eight per wave and step: fp64 distances (wave_dist64_pairs), compared as (d, other) < (d_t, target).
template <typename Dir>
__global__ __launch_bounds__(256) void rank_settle_kernel(const Dir PA, const Dir PB, int nblocks_a, int d) {
  const bool second = (int)blockIdx.x >= nblocks_a;
  const Dir &P = second ? PB : PA;
  const int bid = second ? (int)blockIdx.x - nblocks_a : (int)blockIdx.x;
  const int nbl = second ? (int)gridDim.x - nblocks_a : nblocks_a;
  const int lane = threadIdx.x & 63;
  const unsigned long long offered = *P.pool_n;
  const long long n_e = (long long)(offered < P.cap ? offered : P.cap);
  for (long long e0 = ((long long)bid * 4 + (threadIdx.x >> 6)) * RS_NB; e0 < n_e; e0 += (long long)nbl * 4 * RS_NB) {
    const bool have = lane < RS_NB && e0 + lane < n_e;
    const int2 pr = have ? P.pool[e0 + lane] : make_int2(0, 0);
    int qi[RS_NB], gi[RS_NB];
#pragma unroll
    for (int u = 0; u < RS_NB; ++u) { qi[u] = __shfl(pr.x, u, 64); gi[u] = __shfl(pr.y, u, 64); }
    double dd[RS_NB];
    wave_dist64_pairs(P.own, P.other, qi, gi, d, lane, dd);
    double mine = 0.0;
#pragma unroll
    for (int u = 0; u < RS_NB; ++u) mine = lane == u ? dd[u] : mine;
    if (have) {                                            // (a flagged owner's count is overwritten by rank_brute_kernel, later in the stream)
      const double t = P.dt[pr.x];
      const int tg = rank_target(P, pr.x);
      if (mine < t || (mine == t && pr.y < tg)) atomicAdd(&P.cnt[pr.x], 1);
    }
  }
}

// Flagged owners (their pairs overflowed the pool): the count again, by fp64 brute force over the whole other side; one workgroup of
// eight waves per owner.  Also the statistics: owners sent here, the largest in-reach count of an owner.
template <typename Dir>
__global__ __launch_bounds__(512) void rank_brute_kernel(const Dir PA, const Dir PB, int nblocks_a, int d, unsigned long long *__restrict__ stats) {
  const bool second = (int)blockIdx.x >= nblocks_a;
  const Dir &P = second ? PB : PA;
  const int bid = second ? (int)blockIdx.x - nblocks_a : (int)blockIdx.x;
  const int nbl = second ? (int)gridDim.x - nblocks_a : nblocks_a;
  __shared__ int part[8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int mx = 0;
  // PB is PA transposed (its owners are PA's others): both sizes come from PA, beside nblocks_a in the argument block.  Read through P, the
  // loop bound waits for one more scalar load, behind the one that selects P (+0.002 ms at 10k: a CU runs its workgroups one after another).
  // In a row window PA's owners are the window's rows, so PB counts over exactly those: the rows PA.tgt0 + [0, PA.n_own) of its other side.
  const int n_own = second ? PA.n_other : PA.n_own, n_oth = second ? PA.n_own : PA.n_other, oth0 = second ? PA.tgt0 : 0;
  for (int o = bid; o < n_own; o += nbl) {                   // uniform for the workgroup
    mx = max(mx, P.reach[o]);
    if (!P.ovf[o]) continue;
    const double t = P.dt[o];
    const int tg = rank_target(P, o);
    int cnt = 0;
    for (int j0 = RS_NB * w; j0 < n_oth; j0 += RS_NB * 8) {
      int qi[RS_NB], gi[RS_NB];
#pragma unroll
      for (int u = 0; u < RS_NB; ++u) { qi[u] = o; gi[u] = oth0 + min(j0 + u, n_oth - 1); }
      double dd[RS_NB];
      wave_dist64_pairs(P.own, P.other, qi, gi, d, lane, dd);
#pragma unroll
      for (int u = 0; u < RS_NB; ++u) {
        const int j = oth0 + j0 + u;
        if (j0 + u < n_oth && j != tg && (dd[u] < t || (dd[u] == t && j < tg))) ++cnt;
      }
    }
    if (lane == 0) part[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      int total = 0;
#pragma unroll
      for (int ww = 0; ww < 8; ++ww) total += part[ww];
      P.cnt[o] = total;
      atomicAdd(&stats[4 + (second ? 1 : 0)], 1ull);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && mx) atomicMax(&stats[2 + (second ? 1 : 0)], (unsigned long long)mx);
}

// ---- grouped rank sweep (vtc_l2_rank_grouped): several captions per video ------------------------------------------------------------
// a [n, d] videos, b [m, d] captions, off [n + 1]: the captions of video v are the rows off[v] .. off[v + 1] of b.  The counting sweep above
// made rectangular (D is [m, n]: a caption per row), with the owner's target taken from a table:
//   row direction     owner = caption c, target = its video g(c), d_t = D(c, g(c))                    -> rank_a [m]
//   column direction  owner = video v, target = c* = its own caption with the smallest (D(c, v), c),  -> rank_b [n]
//                     so d_t[v] is the segmented lexicographic minimum of the row direction's d_t over the video's captions
// (include/vtc_hip.h has the definition).  The two kernels below are its own; everything else is the sweep above instantiated with RankDirG.
// Behind them: the video-unit direction (owner = video, other = GROUP of captions), a third pass with kernels of its own.

// g(c) of every caption: the last v with off[v] <= c (an empty group is never the answer: its successor starts at the same caption).
// Whatever `off` holds, the result lies in [0, n).
__global__ __launch_bounds__(256) void rank_group_id_kernel(const int *__restrict__ off, int n, int m, int *__restrict__ gid) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= m) return;
  int lo = 0, hi = n - 1;                                   // invariant: the answer is in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= c) lo = mid; else hi = mid - 1;
  }
  gid[c] = lo;
}

// One thread per video: c* = its own caption with the smallest finite (d_t, c), and the column direction's thresholds.  A video without a
// finite own caption (an empty group too) gets d_t = inf and hi = -inf: rank m.  The columns [n, n_ld) that pad the matrix's rows to
// 16 bytes get hi = -inf too: the column pass neither counts nor pools them.
__global__ __launch_bounds__(256) void rank_grouped_target_kernel(const int *__restrict__ off, int n, int n_ld, int m, const double *__restrict__ dt_r,
                                                                  const float *__restrict__ an2, const float *__restrict__ bmax, float kappa,
                                                                  double *__restrict__ dt_c, int *__restrict__ tgt_c, float *__restrict__ lo_c,
                                                                  float *__restrict__ hi_c) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n_ld) return;
  if (v >= n) {
    dt_c[v] = (double)INFINITY; tgt_c[v] = -1; lo_c[v] = -INFINITY; hi_c[v] = -INFINITY;
    return;
  }
  const int c0 = max(off[v], 0), c1 = min(off[v + 1], m);
  double best = (double)INFINITY;
  int arg = -1;
  for (int c = c0; c < c1; ++c) {
    const double x = dt_r[c];
    if (x < best) { best = x; arg = c; }                // strict: the lower index keeps an exact tie; NaN and inf never enter
  }
  dt_c[v] = best;
  tgt_c[v] = arg;                                       // -1: no row is excluded (and none is counted: hi = -inf)
  const bool ok = arg >= 0;
  const float eps_c = kappa * (an2[v] + *bmax);
  lo_c[v] = ok ? __double2float_rd(best - (double)eps_c) : -INFINITY;
  hi_c[v] = ok ? __double2float_ru(best + (double)eps_c) : -INFINITY;
}

// ---- video-unit direction of the grouped sweep (vtc_l2_rank_grouped_vunit) --------------------------------------------------------------
// owner = video v (a column of D), other = GROUP u (the rows off[u] .. off[u + 1]): E(u, v) = the smallest finite D(c, v) of the group, and
// rank_v[v] = #{ u != v : (E(u, v), u) < (d_t[v], v) } with d_t the column direction's (E(v, v) = D(c*, v)).  A third pass over the same
// distance block classifies every (group, column) ONCE, from the group's smallest key and a "saw a NaN" bit:
//   min key < lo[v]                        closer for certain: the group is counted
//   else some key <= hi[v], or a NaN       in reach: (v, u) goes to the direction's pool, fp64 over the group's captions decides
// A lane owns (one group, four adjacent columns) and walks the group's rows itself -- the four row sub-lanes of the column pass take four
// neighbouring GROUPS here, so a load instruction of the wave is still four 256-byte row pieces and nothing is folded across lanes before a
// group is classified.  A wave takes a strip of 64 columns and a range of the groups that meet the block.  The one group that is open at the
// block's end leaves its (min key, NaN bit) per column in a carry [n_ld]; the block that sees its end picks them up.  Two carries, taken
// in turn by block parity: the group a block closes and the one it leaves open are different lanes of one launch.
template <int U>
__global__ __launch_bounds__(256) void rank_vunit_count_kernel(const float *__restrict__ dist, int ld, int n_rows, int n_cols, int row_id0, int m,
                                                               int n_strips, int S, const int *__restrict__ off, const int *__restrict__ gid,
                                                               float *__restrict__ carry_key, int *__restrict__ carry_nan, int par,
                                                               const RankDir P) {
  constexpr int V = RS_V;                                 // columns per lane = groups per load instruction of the wave
  __shared__ int2 stage_all[4][RS_STAGE];
  int2 *stage = stage_all[threadIdx.x >> 6];              // wave-private
  int n_st = 0;
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n_strips * S) return;
  const int seg = w / n_strips, strip = w - seg * n_strips;
  // the groups that meet the block (gid lies in [0, n) whatever `off` holds), four per step, the steps dealt to the S waves of a strip
  const int gA = gid[row_id0], gB = max(gA, gid[row_id0 + n_rows - 1]);
  const int quads = (gB - gA + V) / V;
  const int qw = (quads + S - 1) / S;
  const int q_lo = seg * qw, q_hi = min(quads, q_lo + qw);
  if (q_lo >= q_hi) return;                               // wave-uniform
  const int c_strip = strip * 64 + 4 * (lane & 15);
  const bool live = c_strip < n_cols;                     // (n_cols % 4 == 0: the lane's four columns are in or out together)
  const int c = live ? c_strip : 0;                       // a lane past the matrix reads column 0, counts nothing and stores nothing
  const int sub = lane >> 4;
  const int r_end = row_id0 + n_rows;
  float lo[V], hi[V];
  int cnt[V], reach[V];
  rank_col_thresholds(P, c, live, lo, hi, cnt, reach);
  for (int q = q_lo; q < q_hi; ++q) {
    const int u = gA + V * q + sub;                       // the lane's group
    const bool have = u <= gB;                            // (gB <= n - 1: off[u + 1] is an entry of off)
    const int g0 = have ? min(max(off[u], 0), m) : 0, g1 = have ? min(max(off[u + 1], 0), m) : 0;
    const int ra = max(g0, row_id0), rb = min(g1, r_end); // its rows in this block: inside [row_id0, r_end) whatever `off` holds
    float mn[V];
    unsigned nanm = 0;
#pragma unroll
    for (int e = 0; e < V; ++e) mn[e] = INFINITY;
    for (int r = ra; r < rb; r += U) {
      float4 t[U];
#pragma unroll
      for (int k = 0; k < U; ++k)                         // past the group's end its last row again: a minimum does not mind
        t[k] = *reinterpret_cast<const float4 *>(dist + (size_t)(min(r + k, rb - 1) - row_id0) * ld + c);
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const float x[V] = {t[k].x, t[k].y, t[k].z, t[k].w};
#pragma unroll
        for (int e = 0; e < V; ++e) {
          mn[e] = x[e] < mn[e] ? x[e] : mn[e];            // a NaN never enters
          nanm |= x[e] != x[e] ? (1u << e) : 0u;
        }
      }
    }
    unsigned mk = 0;
    if (ra < rb && live) {
      if (g0 < row_id0) {                                 // begun in an earlier block
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float ck = carry_key[(size_t)(par ^ 1) * ld + c + e];
          mn[e] = ck < mn[e] ? ck : mn[e];
          nanm |= carry_nan[(size_t)(par ^ 1) * ld + c + e] ? (1u << e) : 0u;
        }
      }
      if (g1 > r_end) {                                   // open at the block's end: the next block classifies it
#pragma unroll
        for (int e = 0; e < V; ++e) {
          carry_key[(size_t)par * ld + c + e] = mn[e];
          carry_nan[(size_t)par * ld + c + e] = (int)((nanm >> e) & 1u);
        }
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const bool ok = hi[e] != -INFINITY && u != c + e;      // the own group is skipped
          const bool lt = mn[e] < lo[e];
          cnt[e] += (ok && lt) ? 1 : 0;
          const bool in = ok && !lt && (!(mn[e] > hi[e]) || ((nanm >> e) & 1u));
          reach[e] += in ? 1 : 0;
          mk |= in ? (1u << e) : 0u;
        }
      }
    }
    if (__ballot(mk != 0) != 0ull)                         // wave-uniform, rare
      rank_stage_append<V>(P, stage, n_st, mk, lane, [&](int e) { return c + e; }, [&](int) { return u; });
  }
  rank_stage_flush(P, stage, n_st, lane);
  rank_col_commit(P, c, live, sub, cnt, reach);
}

// Is group u closer to video v than v's target?  fp64 over the group's captions, eight at a time, by the sweep's one distance function:
// some finite D(c, v) with (D, u) < (d_t, v).  Wave-uniform arguments and result.
__device__ __forceinline__ bool rank_vunit_closer(const RankDir &P, const int *__restrict__ off, int v, int u, double t, int d, int lane) {
  const int m = P.n_other;
  const int c0 = min(max(off[u], 0), m), c1 = min(max(off[u + 1], 0), m);
  bool closer = false;
  for (int j0 = c0; j0 < c1 && !closer; j0 += RS_NB) {
    int qi[RS_NB], gi[RS_NB];
#pragma unroll
    for (int k = 0; k < RS_NB; ++k) { qi[k] = v; gi[k] = min(j0 + k, c1 - 1); }       // past the end the last caption again
    double dd[RS_NB];
    wave_dist64_pairs(P.own, P.other, qi, gi, d, lane, dd);
#pragma unroll
    for (int k = 0; k < RS_NB; ++k) closer = closer || dd[k] < t || (dd[k] == t && u < v);      // NaN and inf: neither
  }
  return closer;
}

// The pooled (video, group) pairs, one per wave and step.
__global__ __launch_bounds__(256) void rank_vunit_settle_kernel(const RankDir P, const int *__restrict__ off, int d) {
  const int lane = threadIdx.x & 63;
  const unsigned long long offered = *P.pool_n;
  const long long n_e = (long long)(offered < P.cap ? offered : P.cap);
  for (long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); e < n_e; e += (long long)gridDim.x * 4) {
    const int2 pr = P.pool[e];
    const int v = __builtin_amdgcn_readfirstlane(pr.x), u = __builtin_amdgcn_readfirstlane(pr.y);
    if (rank_vunit_closer(P, off, v, u, P.dt[v], d, lane) && lane == 0) atomicAdd(&P.cnt[v], 1);
  }
}

// Flagged videos (their pairs overflowed the pool): the count again, by fp64 brute force over all captions, group by group; one workgroup
// of eight waves per video.  Also the direction's statistics (stats[1]: the largest in-reach count of a video, stats[2]: videos sent here).
__global__ __launch_bounds__(512) void rank_vunit_brute_kernel(const RankDir P, const int *__restrict__ off, int d,
                                                               unsigned long long *__restrict__ stats) {
  __shared__ int part[8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n = P.n_own;
  int mx = 0;
  for (int o = blockIdx.x; o < n; o += gridDim.x) {        // uniform for the workgroup
    mx = max(mx, P.reach[o]);
    if (!P.ovf[o]) continue;
    const double t = P.dt[o];
    int cnt = 0;
    for (int u = w; u < n; u += 8) {
      if (u != o && rank_vunit_closer(P, off, o, u, t, d, lane)) ++cnt;
    }
    if (lane == 0) part[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      int total = 0;
#pragma unroll
      for (int ww = 0; ww < 8; ++ww) total += part[ww];
      P.cnt[o] = total;
      atomicAdd(&stats[2], 1ull);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && mx) atomicMax(&stats[1], (unsigned long long)mx);
}

// A video without a finite target ranks behind all n groups.
__global__ __launch_bounds__(256) void rank_vunit_write_kernel(const double *__restrict__ dt_c, const int *__restrict__ cnt_v, int n,
                                                               int64_t *__restrict__ rank_v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) rank_v[i] = dt_c[i] < (double)INFINITY ? (int64_t)cnt_v[i] : (int64_t)n;
}

// ---- both forms: the finish, the workspace and the driver -----------------------------------------------------------------------------
// A caption (row direction, n_r owners) without a finite target distance ranks behind all n videos, a video (column direction) behind all m
// captions.  In a row window the column counts are PARTIAL -- summed over the windows that tile the rows they are rank_b -- so that rank m
// is written by one window only, the one that holds the video's own row [own0, own1); the others write 0.  (Everywhere else the
// range is all n columns.)
__global__ __launch_bounds__(256) void rank_write_kernel(const double *__restrict__ dt_r, const double *__restrict__ dt_c, const int *__restrict__ cnt_r,
                                                         const int *__restrict__ cnt_c, int n, int m, int n_r, int own0, int own1,
                                                         int64_t *__restrict__ rank_a, int64_t *__restrict__ rank_b) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_r) rank_a[i] = dt_r[i] < (double)INFINITY ? (int64_t)cnt_r[i] : (int64_t)n;
  if (i < n) rank_b[i] = dt_c[i] < (double)INFINITY ? (int64_t)cnt_c[i] : (i >= own0 && i < own1) ? (int64_t)m : (int64_t)0;
}

// The workspace of both forms: a [n, d] (the columns of D), b [m, d] (its rows; paired: m = n).  A row of D has n_ld = n rounded up to 4
// columns, so the GEMM writes and both passes read 16-byte aligned rows at every n (measured with ld = n at 2 990 x 20: 1.70 against
// 1.44 ms, profiles/r11_grouped_rank.md); the column-side arrays have n_ld entries, the padding columns zero operands and hi = -inf.
// A row window (vtc_l2_rank_shard: the call owns the rows [w0, w0 + wn) of D; everywhere else wn = m): what belongs to the row direction
// and the rows' operands have wn entries, indexed from the window's first row.  The norms and the pairs' distances are kept for all m rows
// (max |b|^2 and the column direction's thresholds are those of the whole matrix).
struct RankWs {
  unsigned long long *stats;       // [RS_STATS]
  float *qn, *gn, *qmax, *gmax;    // queries = b (m rows of D), gallery = a (n columns)
  bf16_t *qb, *gb;                 // [wn], [n_ld] operand rows
  float *dist;
  int rows_per_block, n_ld;
  int *gid, *tgt_c;                // table form only: [m] g(c); [n_ld] c*
  double *dt_r, *dt_c;             // [m]; table form: [n_ld]; paired: dt_c = dt_r, the pair's distance -- n entries, none for the padding columns
  float *lo_r, *hi_r, *lo_c, *hi_c;      // [wn], [n_ld]
  int *zero;                       // cnt_r, reach_r, ovf_r: [3][wn], then cnt_c, reach_c, ovf_c: [3][n_ld], zeroed by rank_prep_kernel
  int2 *pool_r, *pool_c;
  size_t cap_r, cap_c;
  // video-unit direction only (vtc_l2_rank_grouped_vunit): O(n) words and its pool
  int *zero_v;                     // cnt_v, reach_v, ovf_v: [3][n_ld], behind `zero` and zeroed with it
  float *carry_key;                // [2][n_ld] smallest key of the group that is open at a block's end, by block parity
  int *carry_nan;                  // [2][n_ld] its NaN bit
  int2 *pool_v;
  size_t cap_v;
  size_t total;
};
// default pool: 512 pairs per owner and direction (8 bytes each).  Measured (profiles/r10_rank_sweep.md): an owner in the bulk of unrelated
// unit vectors at d = 512 has 0.216 % of the other side in reach (108 pairs at 50k, at most 203), one whose target leads almost none.
size_t rank_default_capacity(int n) { return std::max<size_t>(4096, (size_t)512 * n); }
RankWs rank_plan(char *ws, int n, int m, int d, int rows_per_block, int reach_capacity, bool table, bool vunit = false, int wn = -1) {
  RankWs s;
  if (wn < 0) wn = m;                                      // no window: every row
  Bump b(ws);
  auto take = [&](size_t bytes) { return b.take(bytes); };
  s.stats = (unsigned long long *)take((RS_STATS + RS_STATS_V) * 8);      // (one 256-byte unit with or without the second eight)
  const int n_ld = (n + 3) & ~3;
  s.n_ld = n_ld;
  s.qn = (float *)take((size_t)m * 4);
  s.gn = (float *)take((size_t)n_ld * 4);
  s.qmax = (float *)take(4);
  s.gmax = (float *)take(4);
  s.qb = (bf16_t *)take((size_t)wn * d * 3 * 2);
  s.gb = (bf16_t *)take((size_t)n_ld * d * 3 * 2);
  s.rows_per_block = std::min(wn, rows_per_block > 0 ? rows_per_block : default_rows_per_block(n_ld));
  s.dist = (float *)take((size_t)s.rows_per_block * n_ld * 4);
  s.gid = table ? (int *)take((size_t)m * 4) : nullptr;
  s.tgt_c = table ? (int *)take((size_t)n_ld * 4) : nullptr;
  s.dt_r = (double *)take((size_t)m * 8);
  s.dt_c = table ? (double *)take((size_t)n_ld * 8) : s.dt_r;
  s.lo_r = (float *)take((size_t)wn * 4);
  s.hi_r = (float *)take((size_t)wn * 4);
  s.lo_c = (float *)take((size_t)n_ld * 4);
  s.hi_c = (float *)take((size_t)n_ld * 4);
  s.zero = (int *)take(((size_t)3 * wn + (size_t)(vunit ? 6 : 3) * n_ld) * 4);
  s.zero_v = vunit ? s.zero + 3 * (size_t)wn + 3 * (size_t)n_ld : nullptr;
  s.cap_r = reach_capacity > 0 ? (size_t)reach_capacity : rank_default_capacity(wn);     // per direction: 512 pairs per OWNER
  s.cap_c = reach_capacity > 0 ? (size_t)reach_capacity : rank_default_capacity(n);
  s.pool_r = (int2 *)take(s.cap_r * 8);
  s.pool_c = (int2 *)take(s.cap_c * 8);
  s.cap_v = s.cap_c;
  s.carry_key = vunit ? (float *)take((size_t)2 * n_ld * 4) : nullptr;
  s.carry_nan = vunit ? (int *)take((size_t)2 * n_ld * 4) : nullptr;
  s.pool_v = vunit ? (int2 *)take(s.cap_v * 8) : nullptr;
  s.total = b.off;
  return s;
}

// All entry points: Dir = RankDir (off == nullptr, m == n) or RankDirG.  The policy decides the prologue's target step and nothing after it.
// rank_v != nullptr (RankDirG, a plan with the video-unit arrays): the video-unit direction rides along, a third pass over every block.
// [w0, w0 + wn): the rows of D this call sweeps (RankDir only, a plan made for wn; everything but vtc_l2_rank_shard passes 0, m).  The row
// direction then has wn owners, numbered from w0 (its arrays and rank_a have wn entries), and the column direction counts every column
// over those rows alone: rank_b holds partial counts that add up over windows that tile the rows (rank_write_kernel).  The blocks carry
// global row ids, the thresholds are those of the whole matrix, so a window settles exactly the whole sweep's pairs that lie in it.
template <typename Dir>
int rank_sweep_impl(const char *fn, const float *a, const float *b, const int *off, int n, int m, int w0, int wn, int d, int64_t *rank_a,
                    int64_t *rank_b, int *nonfinite, const RankWs &s, hipStream_t stream, int64_t *rank_v = nullptr) {
  constexpr bool table = rank_has_table<Dir>;
  const int n_ld = s.n_ld;
  int *cnt_r = s.zero, *reach_r = s.zero + (size_t)wn, *ovf_r = s.zero + 2 * (size_t)wn;
  int *cnt_c = s.zero + 3 * (size_t)wn, *reach_c = cnt_c + (size_t)n_ld, *ovf_c = cnt_c + 2 * (size_t)n_ld;
  auto dir = [](const RankDir &p, const int *tgt) {
    if constexpr (table) return RankDirG{p, tgt};
    else return p;
  };
  // gallery a, query b_c: the rows of D (wn owners from row w0, n others);  gallery b, query a_v: its columns (n owners, the wn rows as others,
  // under their global ids)
  const RankDir r{b + (size_t)w0 * d, a, s.lo_r, s.hi_r, cnt_r, reach_r, ovf_r, s.pool_r, s.stats + 0, (unsigned long long)s.cap_r, s.dt_r + w0, wn, n, w0};
  const RankDir c{a, b, s.lo_c, s.hi_c, cnt_c, reach_c, ovf_c, s.pool_c, s.stats + 1, (unsigned long long)s.cap_c, s.dt_c, n, wn, 0};
  const Dir R = dir(r, s.gid), Cd = dir(c, s.tgt_c);
  // owner = video v, other = GROUP u: the column direction's thresholds and target distance, counters and a pool of its own
  int *cnt_v = s.zero_v, *reach_v = rank_v ? cnt_v + (size_t)n_ld : nullptr, *ovf_v = rank_v ? cnt_v + 2 * (size_t)n_ld : nullptr;
  const RankDir vu{a, b, s.lo_c, s.hi_c, cnt_v, reach_v, ovf_v, s.pool_v, s.stats + RS_STATS, (unsigned long long)s.cap_v, s.dt_c, n, m, 0};
  (void)hipMemsetAsync(s.stats, 0, (RS_STATS + (rank_v ? RS_STATS_V : 0)) * 8, stream);
  (void)hipMemsetAsync(nonfinite, 0, sizeof(int), stream);
  if (int rc = vtc_nonfinite_flag2(a, (size_t)n * d, b, (size_t)m * d, nonfinite, stream)) return rc;
  if (n_ld != n) {                                         // the padding columns' operands: zero rows, zero norms (their entries are never counted)
    (void)hipMemsetAsync(s.gb + (size_t)n * d * 3, 0, (size_t)(n_ld - n) * d * 3 * 2, stream);
    (void)hipMemsetAsync(s.gn + n, 0, (size_t)(n_ld - n) * 4, stream);
  }
  {
    ProfScope prof(VTC_PROF_TOPK, (double)(n + m) * d * (4 + 6 + 4), stream);
    prof.tag(101, m, d);
    const float kappa = split_kappa(d);
    const RankThresholds tr{s.qn + w0, s.gmax, s.dt_r + w0, s.lo_r, s.hi_r}, tc{s.gn, s.qmax, s.dt_c, s.lo_c, s.hi_c};
    if constexpr (table) hipLaunchKernelGGL(rank_group_id_kernel, dim3(cdiv(m, 256)), dim3(256), 0, stream, off, n, m, s.gid);
    launch_norms_split(b, m, s.qn, s.qb, a, n, s.gn, s.gb, d, 3, stream, w0, wn);      // every norm (max |b|^2 is the whole matrix's), the window's operand rows
    hipLaunchKernelGGL(rank_max_kernel, dim3(2), dim3(256), 0, stream, s.gn, n, s.qn, m, s.gmax, s.qmax);
    hipLaunchKernelGGL(rank_prep_kernel<Dir>, dim3(cdiv(cdiv(m, RS_NB), 4)), dim3(256), 0, stream, R, b, m, tr, tc, n_ld, d, kappa, s.zero,
                       3 * wn + (rank_v ? 6 : 3) * n_ld);
    if constexpr (table)
      hipLaunchKernelGGL(rank_grouped_target_kernel, dim3(cdiv(n_ld, 256)), dim3(256), 0, stream, off, n, n_ld, m, s.dt_r, s.gn, s.qmax, kappa, s.dt_c,
                         s.tgt_c, s.lo_c, s.hi_c);
  }
  VTC_LAUNCH_CHECK2(fn, "prologue");
  // D is [rows, n_ld].  The row pass scans the n real columns; the column pass takes all n_ld.
  const int n_strips = cdiv(n_ld, 64);
  for (int r0 = w0; r0 < w0 + wn; r0 += s.rows_per_block) {      // r0: the block's first row of D; r0 - w0: the row direction's owner, the operand row
    const int rows = min(s.rows_per_block, w0 + wn - r0);
    GemmEpi e;
    e.mode = EPI_L2DIST; e.out_dtype = VTC_F32; e.rown = s.qn + r0; e.coln = s.gn;
    if (int rc = launch_gemm(s.qb + (size_t)(r0 - w0) * d * 3, s.gb, nullptr, s.dist, rows, n_ld, d * 3, VTC_BF16, e, stream)) return rc;
    {
      const auto [S, seg_cols] = row_segments(rows, n);
      ProfScope prof(VTC_PROF_TOPK, (double)rows * n * 4, stream);
      prof.tag(102, rows, n);
      hipLaunchKernelGGL(rank_row_count_kernel<Dir>, dim3(cdiv(rows * S, 4)), dim3(256), 0, stream, s.dist, n_ld, rows, n, r0 - w0, S, seg_cols, R);
    }
    {
      // (strip, segment) waves: ~32 per CU; a segment is a whole number of the wave's steps of 8 loads x 4 rows
      const int seg_rows = cdiv(cdiv(rows, std::max(1, cdiv(32 * vtcgemm::num_cus(), n_strips))), 32) * 32;
      const int S = cdiv(rows, seg_rows);
      ProfScope prof(VTC_PROF_TOPK, (double)rows * n * 4, stream);
      prof.tag(103, rows, n);
      hipLaunchKernelGGL(rank_col_count_kernel<Dir>, dim3(cdiv(n_strips * S, 4)), dim3(256), 0, stream, s.dist, n_ld, rows, n_ld, r0, n_strips, S, seg_rows, Cd);
    }
    if (rank_v) {
      // (strip, range of groups) waves: ~32 per CU; the groups that meet the block are counted on the device
      const int S = std::max(1, std::min(cdiv(n, 4), cdiv(32 * vtcgemm::num_cus(), n_strips)));
      ProfScope prof(VTC_PROF_TOPK, (double)rows * n * 4, stream);
      prof.tag(106, rows, n);
      hipLaunchKernelGGL(rank_vunit_count_kernel<4>, dim3(cdiv(n_strips * S, 4)), dim3(256), 0, stream, s.dist, n_ld, rows, n_ld, r0, m, n_strips, S,
                         off, s.gid, s.carry_key, s.carry_nan, (r0 / s.rows_per_block) & 1, vu);
    }
    VTC_LAUNCH_CHECK2(fn, "count");
  }
  if (rank_v) {
    ProfScope prof(VTC_PROF_TOPK, 0.0, stream);
    prof.tag(107, n, d);
    hipLaunchKernelGGL(rank_vunit_settle_kernel, dim3((int)std::min<size_t>(2048, (s.cap_v + 3) / 4)), dim3(256), 0, stream, vu, off, d);
    hipLaunchKernelGGL(rank_vunit_brute_kernel, dim3(std::min(n, 1024)), dim3(512), 0, stream, vu, off, d, s.stats + RS_STATS);
    hipLaunchKernelGGL(rank_vunit_write_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, s.dt_c, cnt_v, n, rank_v);
  }
  {
    // eight pairs per wave and step; the pools' fill lives on the device, so the grid is sized for a full pool and strides
    const int ga = (int)std::min<size_t>(2048, (s.cap_r + 4 * RS_NB - 1) / (4 * RS_NB));
    const int gb = (int)std::min<size_t>(2048, (s.cap_c + 4 * RS_NB - 1) / (4 * RS_NB));
    ProfScope prof(VTC_PROF_TOPK, 0.0, stream);
    prof.tag(104, m, d);
    hipLaunchKernelGGL(rank_settle_kernel<Dir>, dim3(ga + gb), dim3(256), 0, stream, R, Cd, ga, d);
  }
  {
    const int ga = std::min(wn, 1024), gb = std::min(n, 1024);
    ProfScope prof(VTC_PROF_TOPK, 0.0, stream);
    prof.tag(105, m, d);
    hipLaunchKernelGGL(rank_brute_kernel<Dir>, dim3(ga + gb), dim3(512), 0, stream, R, Cd, ga, d, s.stats);
  }
  hipLaunchKernelGGL(rank_write_kernel, dim3(cdiv(std::max(n, wn), 256)), dim3(256), 0, stream, s.dt_r + w0, s.dt_c, cnt_r, cnt_c, n, m, wn, table ? 0 : w0,
                     table ? n : w0 + wn, rank_a, rank_b);
  VTC_LAUNCH_CHECK2(fn, "finish");
  return 0;
}
}  // namespace

// ---- full ranks of both directions (median / mean rank, MRR, recall at any k): include/vtc_hip.h ----------------------------
extern "C" float vtc_l2_rank_kappa(int d) { return split_kappa(d); }

// what every entry point asks of its arguments (m < 0: the paired form, which has no m)
static int rank_check_args(const char *fn, bool no_null, int n, int m, int d, int reach_capacity) {
  VTC_CHECK(no_null, "%s: null argument", fn);
  VTC_CHECK(n >= 1, "%s: n=%d must be >= 1", fn, n);
  VTC_CHECK(m < 0 || m >= 1, "%s: m=%d must be >= 1", fn, m);
  VTC_CHECK(d > 0 && d % 64 == 0, "%s: d=%d must be a positive multiple of 64", fn, d);
  VTC_CHECK(reach_capacity >= 0, "%s: reach_capacity=%d must be >= 0 (0: the default)", fn, reach_capacity);
  return 0;
}
extern "C" size_t vtc_l2_rank_bidir_workspace_bytes(int n, int d, int rows_per_block, int reach_capacity) {
  if (n < 1 || d < 1) return 0;
  return rank_plan(nullptr, n, n, d, rows_per_block, reach_capacity, false).total;
}
extern "C" int vtc_l2_rank_bidir(const float *a, const float *b, int n, int d, int rows_per_block, int reach_capacity, int64_t *rank_a,
                                 int64_t *rank_b, int *nonfinite, void *ws, size_t ws_bytes, void *stream) {
  if (int rc = rank_check_args("l2_rank_bidir", a && b && rank_a && rank_b && nonfinite, n, -1, d, reach_capacity)) return rc;
  const RankWs s = rank_plan((char *)ws, n, n, d, rows_per_block, reach_capacity, false);
  VTC_CHECK(ws && ws_bytes >= s.total, "l2_rank_bidir: workspace too small (%zu < %zu)", ws_bytes, s.total);
  return rank_sweep_impl<RankDir>("l2_rank_bidir", a, b, nullptr, n, n, 0, n, d, rank_a, rank_b, nonfinite, s, (hipStream_t)stream);
}

// ---- the paired sweep over a window of rows (one rank of a row-sharded evaluation): include/vtc_hip.h -------------------------------
extern "C" size_t vtc_l2_rank_shard_workspace_bytes(int n_total, int n_local, int d, int rows_per_block, int reach_capacity) {
  if (n_total < 1 || d < 1 || n_local < 0 || n_local > n_total) return 0;
  return rank_plan(nullptr, n_total, n_total, d, rows_per_block, reach_capacity, false, false, n_local).total;
}
extern "C" int vtc_l2_rank_shard(const float *a_all, const float *b_all, int n_total, int row_base, int n_local, int d, int rows_per_block,
                                 int reach_capacity, int64_t *rank_a_local, int64_t *rank_b_part, int *nonfinite, void *ws, size_t ws_bytes,
                                 void *stream) {
  if (int rc = rank_check_args("l2_rank_shard", a_all && b_all && rank_a_local && rank_b_part && nonfinite, n_total, -1, d, reach_capacity)) return rc;
  VTC_CHECK(row_base >= 0 && n_local >= 0 && (long long)row_base + n_local <= n_total,
            "l2_rank_shard: window row_base=%d, n_local=%d must lie in [0, n_total=%d]", row_base, n_local, n_total);
  const RankWs s = rank_plan((char *)ws, n_total, n_total, d, rows_per_block, reach_capacity, false, false, n_local);
  VTC_CHECK(ws && ws_bytes >= s.total, "l2_rank_shard: workspace too small (%zu < %zu)", ws_bytes, s.total);
  return rank_sweep_impl<RankDir>("l2_rank_shard", a_all, b_all, nullptr, n_total, n_total, row_base, n_local, d, rank_a_local, rank_b_part, nonfinite,
                                  s, (hipStream_t)stream);
}

extern "C" size_t vtc_l2_rank_grouped_workspace_bytes(int n, int m, int d, int rows_per_block, int reach_capacity) {
  if (n < 1 || m < 1 || d <= 0 || reach_capacity < 0) return 0;
  return rank_plan(nullptr, n, m, d, rows_per_block, reach_capacity, true).total;
}
extern "C" int vtc_l2_rank_grouped(const float *a, const float *b, const int *off, int n, int m, int d, int rows_per_block, int reach_capacity,
                                   int64_t *rank_a, int64_t *rank_b, int *nonfinite, void *ws, size_t ws_bytes, void *stream) {
  if (int rc = rank_check_args("l2_rank_grouped", a && b && off && rank_a && rank_b && nonfinite, n, m, d, reach_capacity)) return rc;
  const RankWs s = rank_plan((char *)ws, n, m, d, rows_per_block, reach_capacity, true);
  VTC_CHECK(ws && ws_bytes >= s.total, "l2_rank_grouped: workspace too small (%zu < %zu)", ws_bytes, s.total);
  return rank_sweep_impl<RankDirG>("l2_rank_grouped", a, b, off, n, m, 0, m, d, rank_a, rank_b, nonfinite, s, (hipStream_t)stream);
}

extern "C" size_t vtc_l2_rank_grouped_vunit_workspace_bytes(int n, int m, int d, int rows_per_block, int reach_capacity) {
  if (n < 1 || m < 1 || d <= 0 || reach_capacity < 0) return 0;
  return rank_plan(nullptr, n, m, d, rows_per_block, reach_capacity, true, true).total;
}
extern "C" int vtc_l2_rank_grouped_vunit(const float *a, const float *b, const int *off, int n, int m, int d, int rows_per_block,
                                         int reach_capacity, int64_t *rank_a, int64_t *rank_b, int64_t *rank_v, int *nonfinite, void *ws,
                                         size_t ws_bytes, void *stream) {
  if (int rc = rank_check_args("l2_rank_grouped_vunit", a && b && off && rank_a && rank_b && rank_v && nonfinite, n, m, d, reach_capacity)) return rc;
  const RankWs s = rank_plan((char *)ws, n, m, d, rows_per_block, reach_capacity, true, true);
  VTC_CHECK(ws && ws_bytes >= s.total, "l2_rank_grouped_vunit: workspace too small (%zu < %zu)", ws_bytes, s.total);
  return rank_sweep_impl<RankDirG>("l2_rank_grouped_vunit", a, b, off, n, m, 0, m, d, rank_a, rank_b, nonfinite, s, (hipStream_t)stream, rank_v);
}
