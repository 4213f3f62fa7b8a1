// sweep_recall.hip -- the recall-only finish of the block-minima sweep: R@K hit counters from the RANK of each query's target, without
// the sorted lists.
//   vtc_l2_recall_bidir                 both directions of n paired rows on one GPU
//   vtc_l2_recall_shard_rows / _cols    the same with the rows sharded one process per GPU; vtc_l2_recall_planes: the planes that travel
// Prologue, workspace and the distance GEMM's key planes are the block-minima path's (sweep_front.hip, gemm.hip); the sorted-list sweep is
// sweep_topk.hip.
#include "sweep_common.h"

#include <algorithm>

using namespace vtcsweep;

namespace {

// ---- recall-only finish of the block-minima sweep (round 5) ----------------------------------------------------------------
// The reference's RecallAtK.compute (model/metric.py:137-161) searches the max(k)+1 nearest gallery rows of every query and then asks
// ONE thing of the sorted list: is the query's own row index among the first k.  That is the RANK of one gallery row,
//     rank_i = #{ j : (|q_i - g_j|^2, j) < (|q_i - g_t|^2, t) },  t = the query's target,        hit at k  <=>  rank_i < k
// (ties by lowest index, as in every sweep), and it does not need the sorted top list.  From the key planes of the distance
// GEMM: with d_t the target's exact fp64 distance and eps the row's bound on |key distance - exact| (the formula of sweep_topk.hip's minsel_kernel),
//   key + eps < d_t   the entry is closer for certain         key - eps > d_t   farther for certain         else: fp64 decides;
// a block whose FOURTH-smallest key is <= d_t + eps may hide unlisted entries in reach of d_t: all its entries go to fp64.
// If the certain ones alone number >= max(k) the query misses at every k and nothing else is looked at -- the fate of most queries of
// an untrained model -- and for a query whose target leads its list (a trained model) almost nothing is in reach: the fp64 re-rank of
// ~20 candidate rows per query (the sweep's largest consumer of bytes) shrinks to the target row and a handful.  Same hits as
// vtc_l2_topk_bidir + vtc_recall_hits_pair, bit for bit in the counters.
// What the recall-only sweep asks of the distance GEMM (gemm.hip, l2min_epilogue).  max(k) <= 16 and many blocks per row (>= 16 384 rows): the
// block's smallest key + the second as a bound in both directions (EPI_L2MIN2: 6 vector instructions per value, half the plane bytes) -- a block
// with two entries in reach of a target goes to fp64 whole, which for a target with r closer entries happens about r^2 / (2 x blocks) of the time:
// rare at 50k (782 / 391 blocks).  At 10k (157 / 79 blocks) it is not, and the COLUMN direction -- blocks of 128 rows: twice as likely and twice
// as dear as the rows' blocks of 64 -- made the finish kernel 93 us of a 0.3 ms sweep on low-recall data: there the columns keep two keys + bound
// (EPI_L2MIN3: rows two planes, columns three; 7 per value).  max(k) > 16: three keys + bound in both.
static int recall_mode(int kmax, int n_total) {
  if (kmax > 16) return EPI_L2MIN;
  return n_total < 16384 ? EPI_L2MIN3 : EPI_L2MIN2;
}
struct RecallArgs {
  const unsigned *keys;        // [nsrc][NPL][nblk][R], NPL = 4 (EPI_L2MIN: three keys + bound) or 2 (EPI_L2MIN2: one key + bound) -- the kernel's template argument
  int R, nblk, bw;             // owners (queries of this direction), blocks PER SOURCE, entries per block (64 rows / RB columns)
  int nsrc;                    // sources of key planes: 1, or (sharded sweep, column direction) the ranks that each ran a [rows of theirs, R] GEMM
  const int *bounds;           // [nsrc + 1] (device): source s covers the other side's rows [bounds[s], bounds[s + 1]); NULL: one source, [0, ng)
  int tgt_off;                 // owner r is paired with row r + tgt_off of the other side (sharded sweep: the rank's first row; else 0)
  const float *own, *other;    // fp32 rows: [R, d] owners, [ng, d] the other side
  int ng, d;
  const float *own_norm;
  const float2 *own_st;
  const float *other_max;
  float kappa;
  int kmax, nk, k[4];
  unsigned long long *hits;    // [nk], added to
  int *flags;                  // flags[0] = count, flags[1..] = rows left to recall_rank_finish_kernel: r (lists overflowed: brute force) or r | RK_HARD
  int *work;                   // [R][RK_WORK] ints: a deferred row's (closer_safe, n_amb, n_ub, unsafe blocks' first entry[RK_UB] and end[RK_UB], ambiguous entries[RK_AMB])
  int *part;                   // [workgroups of recall_rank_kernel][4]: their hit counts, summed by recall_rank_finish_kernel (one atomic per k
                               // instead of one per wave: 7 500 same-address atomics were 75 of the kernel's 125 us at 10k)
  int nparts;
};
constexpr int RK_OW = 32, RK_CH = 64, RK_AMB = 64, RK_UB = 8;      // owners per workgroup, blocks per chunk, list capacities per owner
constexpr int RK_WORK = 128, RK_HARD = 1 << 30, RK_INLINE = 16;      // ints per deferred row; flag bit; fp64 evaluations a wave does inline
constexpr int RK_TLS = RK_CH * (RK_OW + 1);           // words of one plane's tile in LDS
// A row whose target distance is non-finite adds this to its workgroup's FIRST partial hit count (a workgroup owns RK_OW = 32 rows: the
// real count stays below it); the finish kernel strips it and raises bit 40 of the direction's first counter instead (VTC_RECALL_NONFINITE,
// include/vtc_hip.h) -- the caller learns of NaN / inf embeddings from the counters it reads anyway, without another launch.
constexpr int RK_NONFINITE = 1 << 20;
template <int MAXP>      // planes of the wider of the kernel's two directions: 27 KiB of LDS with two planes (five workgroups per CU), 44 with four (three)
struct RecallShared {
  unsigned tl[MAXP * RK_TLS];
  int amb[RK_OW][RK_AMB];
  int ublk[RK_OW][RK_UB], uend[RK_OW][RK_UB];       // unsafe blocks: first entry and end (the block's or its source's)
  int hsum[4][4];
};
// one direction's workgroup; NPL = planes of ITS key layout (the two directions of one sweep may differ: gemm.hip, EPI_L2MIN3)
template <int NPL, typename Shared>
__device__ __forceinline__ void recall_rank_body(const RecallArgs &P, int bid, Shared &sh) {
  const int R = P.R, nblk = P.nblk, bw = P.bw, ng = P.ng, d = P.d, kmax = P.kmax;
  unsigned *tl = sh.tl;
  auto &amb = sh.amb;
  auto &ublk = sh.ublk;
  auto &uend = sh.uend;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int toff = P.tgt_off;
  constexpr int OPW = RK_OW / 4;                     // owners per wave
  const int r0 = bid * RK_OW;
  const size_t plane = (size_t)nblk * R;
  // ---- the targets' exact distances and the rows' thresholds (wave-uniform per owner) ----
  double dt[OPW];
  float lo[OPW], hi[OPW];
  {
    // the wave's eight (owner, target) pairs at once (one pair at a time this was eight dependent gather + butterfly latencies: 100 of the
    // kernel's 123 us at 10k); target of owner r: row r + tgt_off of the other side
    int qi[OPW], gi[OPW];
#pragma unroll
    for (int cc = 0; cc < OPW; ++cc) {
      qi[cc] = min(r0 + OPW * w + cc, R - 1);
      gi[cc] = min(qi[cc] + toff, ng - 1);
    }
    wave_dist64_pairs(P.own, P.other, qi, gi, d, lane, dt);
#pragma unroll
    for (int cc = 0; cc < OPW; ++cc) {
      const int r = min(r0 + OPW * w + cc, R - 1);
      const float2 st = P.own_st[r];
      const float eps = 1.001f * (2.0f * (st.x * P.other_max[2] + st.y * P.other_max[1] + st.y * P.other_max[2]) + P.kappa * (P.own_norm[r] + P.other_max[0]));
      // (two / three planes: the keys are HALF distances -- gemm.hip, EPI_L2MIN2 -- and so are the thresholds; halving is exact)
      constexpr double KS = NPL != 4 ? 0.5 : 1.0;
      lo[cc] = __double2float_rd(KS * (dt[cc] - (double)eps));      // key <  lo  =>  key + eps < d_t
      hi[cc] = __double2float_ru(KS * (dt[cc] + (double)eps));      // key >  hi  =>  key - eps > d_t
    }
  }
  // per LANE (= block of the chunk) counters, reduced over the wave once behind the scan: a ballot + population count per (owner, plane,
  // chunk) for each of them made the scan vector-ALU-bound (17 us per chunk of 64 blocks; 0.9 ms of the 50k sweep)
  int ca_l[OPW], cs_l[OPW], n_amb[OPW], n_ub[OPW];
#pragma unroll
  for (int cc = 0; cc < OPW; ++cc) ca_l[cc] = cs_l[cc] = n_amb[cc] = n_ub[cc] = 0;
  const int so = t % RK_OW, sb = t / RK_OW;          // scalar tile loads: this thread's owner and block slice (8 slices)
  const bool vec = (R & 3) == 0;                      // 16-byte loads: four consecutive owners per thread, 8 threads per (plane, block) row
  const int vo = 4 * (t & 7), vb = t >> 3;            // ... this thread's first owner and (block, plane) slice: 32 slices
  for (int src = 0; src < P.nsrc; ++src) {
  const int sbeg = P.bounds ? P.bounds[src] : 0, send = P.bounds ? P.bounds[src + 1] : ng;
  const unsigned *__restrict__ keys = P.keys + (size_t)src * NPL * plane;
  for (int c0 = 0; c0 < nblk; c0 += RK_CH) {
    if (vec) {
      uint4 v[RK_CH * NPL / 32];
#pragma unroll
      for (int q = 0; q < RK_CH * NPL / 32; ++q) {     // (block, plane) pairs vb + 32 q of the chunk: plane = pair % NPL, block = pair / NPL
        const int pr = vb + 32 * q, pl = pr % NPL, bl = pr / NPL, blk = c0 + bl;
        const bool ok = blk < nblk && r0 + vo < R;
        v[q] = ok ? *reinterpret_cast<const uint4 *>(keys + pl * plane + (size_t)blk * R + r0 + vo) : make_uint4(0x7F800000u, 0x7F800000u, 0x7F800000u, 0x7F800000u);
      }
#pragma unroll
      for (int q = 0; q < RK_CH * NPL / 32; ++q) {
        const int pr = vb + 32 * q, pl = pr % NPL, bl = pr / NPL;
        unsigned *dst = &tl[(pl) * RK_TLS + bl * (RK_OW + 1) + vo];
        dst[0] = v[q].x; dst[1] = v[q].y; dst[2] = v[q].z; dst[3] = v[q].w;
      }
    } else {
#pragma unroll
      for (int q = 0; q < RK_CH / 8; ++q) {
        const int bl = sb + 8 * q, blk = c0 + bl;
        const bool ok = blk < nblk && r0 + so < R;
        const size_t o = ok ? (size_t)blk * R + r0 + so : 0;
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) tl[(pl) * RK_TLS + bl * (RK_OW + 1) + so] = ok ? keys[pl * plane + o] : 0x7F800000u;
      }
    }
    __syncthreads();
    const int blk = c0 + lane;
    const int base = sbeg + blk * bw;
#pragma unroll
    for (int cc = 0; cc < OPW; ++cc) {
      const int o = OPW * w + cc, tg = r0 + o + toff;
      const unsigned k3 = tl[(NPL - 1) * RK_TLS + lane * (RK_OW + 1) + o];            // the block's bound: its NPL-th smallest key
      const bool unsafe = k3 != 0x7F800000u && __uint_as_float(k3 & ~127u) <= hi[cc];
      // the bound is an entry too (the block's NPL-th smallest): closer for certain, it raises the LOWER bound on the rank that ends a query as a
      // miss without any fp64 (with two planes a query whose few closer entries share blocks would otherwise go to fp64 for a rank >= max k)
      ca_l[cc] += (unsafe && __uint_as_float(k3 & ~127u) < lo[cc] && base + (int)(k3 & 127u) != tg) ? 1 : 0;
      unsigned kk[NPL - 1];
      bool am[NPL - 1];
      bool any_am = false;
#pragma unroll
      for (int pl = 0; pl < NPL - 1; ++pl) {
        kk[pl] = tl[(pl) * RK_TLS + lane * (RK_OW + 1) + o];
        const float v = __uint_as_float(kk[pl] & ~127u);
        const bool valid = kk[pl] != 0x7F800000u && base + (int)(kk[pl] & 127u) != tg;     // (the target itself is not counted)
        const bool dc = valid && v < lo[cc];
        am[pl] = valid && !dc && !(v > hi[cc]) && !unsafe;                                  // (an unsafe block's entries all go to fp64 below)
        any_am |= am[pl];
        ca_l[cc] += dc ? 1 : 0;
        cs_l[cc] += (dc && !unsafe) ? 1 : 0;
      }
      const unsigned long long um = __ballot(unsafe);
      if (um) {                                                           // wave-uniform, rare
        const int pos = n_ub[cc] + __popcll(um & ((1ull << lane) - 1ull));
        if (unsafe && pos < RK_UB) { ublk[o][pos] = base; uend[o][pos] = min(base + bw, send); }
        n_ub[cc] += __popcll(um);
      }
      if (__ballot(any_am)) {                                             // wave-uniform, rare: entries within eps of the target's distance
#pragma unroll
        for (int pl = 0; pl < NPL - 1; ++pl) {
          const unsigned long long mask = __ballot(am[pl]);
          const int pos = n_amb[cc] + __popcll(mask & ((1ull << lane) - 1ull));
          if (am[pl] && pos < RK_AMB) amb[o][pos] = base + (int)(kk[pl] & 127u);
          n_amb[cc] += __popcll(mask);
        }
      }
    }
    __syncthreads();
  }
  }
  int closer_all[OPW], closer_safe[OPW];
#pragma unroll
  for (int cc = 0; cc < OPW; ++cc) {
    int x = ca_l[cc], y = cs_l[cc];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { x += __shfl_xor(x, o, 64); y += __shfl_xor(y, o, 64); }
    closer_all[cc] = x; closer_safe[cc] = y;
  }
  // ---- settle: certain misses, fp64 for what is in reach, the rest to the fallback ----
  int hit_cnt[4] = {0, 0, 0, 0};
#pragma unroll
  for (int cc = 0; cc < OPW; ++cc) {
    const int o = OPW * w + cc, r = r0 + o, tg = r + toff;
    if (r >= R) continue;                                                 // wave-uniform
    if (closer_all[cc] >= kmax) continue;                                 // a miss at every k
    // a non-finite target distance (NaN / inf in the query's or its target's embedding): every comparison below would be false and the
    // rank would read 0 -- a hit at every k.  An exact search never returns such a target (no distance compares below NaN): a miss.
    if (!(dt[cc] < (double)INFINITY)) { hit_cnt[0] += RK_NONFINITE; continue; }       // (... and said: recall_rank_finish_kernel raises VTC_RECALL_NONFINITE in the counters)
    if (n_amb[cc] > RK_AMB || n_ub[cc] > RK_UB) {
      if (lane == 0) P.flags[1 + atomicAdd(P.flags, 1)] = r;
      continue;
    }
    if (n_amb[cc] + n_ub[cc] * bw > RK_INLINE) {
      // a row with much in reach of its target (the target sits inside the bulk of its row's distances, yet fewer than max(k) entries are
      // closer for certain): its fp64 work -- every entry of its unsafe blocks -- is a long serial chain for ONE wave that has seven more
      // owners to do (the stragglers were the whole kernel time: 127 us at 10k for 0.3 % of the rows).  Deferred with its lists:
      // recall_rank_finish_kernel gives it a workgroup of its own.
      int *wk = P.work + (size_t)r * RK_WORK;
      if (lane == 0) { wk[0] = closer_safe[cc]; wk[1] = n_amb[cc]; wk[2] = n_ub[cc]; }
      if (lane < n_ub[cc]) { wk[3 + lane] = ublk[o][lane]; wk[3 + RK_UB + lane] = uend[o][lane]; }
      if (lane < n_amb[cc]) wk[3 + 2 * RK_UB + lane] = amb[o][lane];
      if (lane == 0) P.flags[1 + atomicAdd(P.flags, 1)] = r | RK_HARD;
      continue;
    }
    const float *q = P.own + (size_t)r * d;
    int rank = closer_safe[cc];
    auto count_group = [&](const int (&jj)[8]) {
      double dd[8];
      int rows[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) rows[u] = jj[u] < 0 ? 0 : jj[u];      // an absent slot reads row 0; its result is not counted
      wave_dist64_rows(q, P.other, rows, d, lane, dd);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (jj[u] >= 0 && (dd[u] < dt[cc] || (dd[u] == dt[cc] && jj[u] < tg))) ++rank;
    };
    for (int c0 = 0; c0 < n_amb[cc] && rank < kmax; c0 += 8) {
      int jj[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) jj[u] = c0 + u < n_amb[cc] ? amb[o][c0 + u] : -1;
      count_group(jj);
    }
    for (int ub = 0; ub < n_ub[cc] && rank < kmax; ++ub) {
      const int base = ublk[o][ub], end = uend[o][ub];
      for (int c0 = 0; c0 < bw && rank < kmax; c0 += 8) {
        int jj[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int j = base + c0 + u;
          jj[u] = (j < end && j != tg) ? j : -1;
        }
        count_group(jj);
      }
    }
#pragma unroll
    for (int qk = 0; qk < 4; ++qk)
      if (qk < P.nk && rank < P.k[qk]) ++hit_cnt[qk];
  }
  auto &hsum = sh.hsum;
  if (lane == 0) {
#pragma unroll
    for (int qk = 0; qk < 4; ++qk) hsum[w][qk] = hit_cnt[qk];
  }
  __syncthreads();
  if (t < 4) P.part[(size_t)bid * 4 + t] = hsum[0][t] + hsum[1][t] + hsum[2][t] + hsum[3][t];
}
template <int NPLA, int NPLB>
__global__ __launch_bounds__(256) void recall_rank_kernel(const RecallArgs PA, const RecallArgs PB, int nblocks_a) {
  __shared__ RecallShared<(NPLA > NPLB ? NPLA : NPLB)> sh;
  if ((int)blockIdx.x < nblocks_a) recall_rank_body<NPLA>(PA, (int)blockIdx.x, sh);
  else recall_rank_body<NPLB>(PB, (int)blockIdx.x - nblocks_a, sh);
}
// The rows recall_rank_kernel left over, one workgroup per row: a DEFERRED row (r | RK_HARD) comes with its lists -- the waves split its
// fp64 evaluations; a row whose lists overflowed (dense near-ties around the target) gets its rank by fp64 brute force over the other side.
constexpr int RK_FW = 8;        // waves of a finish workgroup: a deferred row is 64 - 128 fp64 distances of 2 KB rows, latency-bound -- eight at once per wave
__global__ __launch_bounds__(64 * RK_FW) void recall_rank_finish_kernel(const RecallArgs PA, const RecallArgs PB, int nblocks_a) {
  const bool second = (int)blockIdx.x >= nblocks_a;
  const RecallArgs &P = second ? PB : PA;
  const int bid = second ? (int)blockIdx.x - nblocks_a : (int)blockIdx.x;
  const int nbl = second ? (int)gridDim.x - nblocks_a : nblocks_a;
  __shared__ int part[RK_FW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (bid == 0) {            // this direction's first workgroup: the rank kernel's per-workgroup hit counts -> one atomic per k
    int acc[4] = {0, 0, 0, 0};
    int nf = 0;
    for (int i = threadIdx.x; i < P.nparts; i += 64 * RK_FW) {
      const int4 v = *reinterpret_cast<const int4 *>(P.part + (size_t)i * 4);
      nf |= v.x >> 20;                                   // rows with a non-finite target distance (RK_NONFINITE each)
      acc[0] += v.x & (RK_NONFINITE - 1); acc[1] += v.y; acc[2] += v.z; acc[3] += v.w;
    }
    if (__ballot(nf != 0) != 0 && lane == 0) atomicOr(&P.hits[0], 1ull << 40);       // VTC_RECALL_NONFINITE
    __shared__ int red[RK_FW][4];
#pragma unroll
    for (int qk = 0; qk < 4; ++qk) {
      int x = acc[qk];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
      if (lane == 0) red[w][qk] = x;
    }
    __syncthreads();
    if ((int)threadIdx.x < P.nk) {
      int x = 0;
#pragma unroll
      for (int ww = 0; ww < RK_FW; ++ww) x += red[ww][threadIdx.x];
      if (x) atomicAdd(&P.hits[threadIdx.x], (unsigned long long)x);
    }
    __syncthreads();
  }
  const int n_flagged = P.flags[0];
  for (int f = bid; f < n_flagged; f += nbl) {          // uniform for the workgroup; normally few trips
    const int fr = P.flags[1 + f];
    const bool hard = (fr & RK_HARD) != 0;
    const int r = fr & ~RK_HARD, tg = r + P.tgt_off;
    const float *q = P.own + (size_t)r * P.d;
    const double dt = wave_dist64(q, P.other + (size_t)tg * P.d, P.d, lane);
    const bool dt_ok = dt < (double)INFINITY;      // (the rank kernel never flags a row with a non-finite target distance; kept for the brute-force form)
    int cnt = 0, base_rank = 0;
    auto count_group = [&](const int (&jj)[8]) {
      double dd[8];
      int rows[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) rows[u] = jj[u] < 0 ? 0 : jj[u];      // an absent slot reads row 0; its result is not counted
      wave_dist64_rows(q, P.other, rows, P.d, lane, dd);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (jj[u] >= 0 && (dd[u] < dt || (dd[u] == dt && jj[u] < tg))) ++cnt;
    };
    if (hard) {
      const int *wk = P.work + (size_t)r * RK_WORK;
      base_rank = wk[0];
      const int n_amb = wk[1], n_ub = wk[2];
      const int n_eval = n_amb + n_ub * P.bw;           // evaluation e: e < n_amb -> ambiguous entry e; else entry (e - n_amb) % bw of unsafe block (e - n_amb) / bw
      for (int e0 = 8 * w; e0 < n_eval; e0 += 8 * RK_FW) {
        int jj[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int e = e0 + u;
          int j = -1;
          if (e < n_amb) j = wk[3 + 2 * RK_UB + e];
          else if (e < n_eval) {
            const int x = e - n_amb, ub = x / P.bw;
            j = wk[3 + ub] + (x - ub * P.bw);
            if (j >= wk[3 + RK_UB + ub] || j == tg) j = -1;
          }
          jj[u] = j;
        }
        count_group(jj);
      }
    } else {
      for (int j0 = 8 * w; j0 < P.ng; j0 += 8 * RK_FW) {
        int jj[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) jj[u] = (j0 + u < P.ng && j0 + u != tg) ? j0 + u : -1;
        count_group(jj);
      }
    }
    if (lane == 0) part[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      int rank = base_rank;
#pragma unroll
      for (int ww = 0; ww < RK_FW; ++ww) rank += part[ww];
#pragma unroll
      for (int qk = 0; qk < 4; ++qk)          // (constant indices: a run-time index into P.k[] sends the argument block to scratch)
        if (qk < P.nk && dt_ok && rank < P.k[qk]) atomicAdd(&P.hits[qk], 1ull);
    }
    __syncthreads();
  }
}

// The ROW direction of a plan2 workspace: the owners are the GEMM's rows (its queries), their keys s.rowk in blocks of 64 rows of the
// other side.  The column direction and the sharded column finish start from this and re-assign, by name, what differs.
RecallArgs recall_args(const Sweep2Ws &s, const float *own, const float *other, int R, int ng, int d, int tgt_off, const KList &kl,
                   unsigned long long *hits) {
  static_assert(RK_WORK * sizeof(int) <= CD2 * sizeof(int64_t) && 3 + 2 * RK_UB + RK_AMB <= RK_WORK, "a deferred row's lists fit its candidate-list slot");
  RecallArgs r;
  r.keys = s.rowk; r.R = R; r.nblk = s.nblk_c; r.bw = 64;
  r.nsrc = 1; r.bounds = nullptr; r.tgt_off = tgt_off;
  r.own = own; r.other = other; r.ng = ng; r.d = d;
  r.own_norm = s.qn; r.own_st = s.qst; r.other_max = s.gmax; r.kappa = exact2_kappa(d);
  r.kmax = kl.kmax; r.nk = kl.nk;
  for (int i = 0; i < 4; ++i) r.k[i] = kl.k[i];
  r.hits = hits; r.flags = s.flags;
  r.work = (int *)s.cand;
  r.part = s.cand_n; r.nparts = cdiv(R, RK_OW);            // (4 ints per workgroup in the cand_n array: R / 8 <= R)
  return r;
}

// recall_rank_kernel + recall_rank_finish_kernel (the fallback launch, normally empty) for one direction (B == nullptr: the second
// argument block is not used, every workgroup is "first") or both in one launch per stage.  npl_*: key planes per block of the direction;
// both directions run as <2, 2>, <2, 3> or <4, 4> (EPI_L2MIN2 / L2MIN3 / L2MIN), a single one as <npl, npl>.
void launch_recall(const RecallArgs &A, int npl_a, const RecallArgs *B, int npl_b, hipStream_t stream) {
  const RecallArgs &Bv = B ? *B : A;
  if (!B) npl_b = npl_a;
  {
    double work = (double)npl_a * A.nsrc * A.nblk * A.R * 4 + 2.0 * A.R * A.d * 4;
    if (B) work += (double)npl_b * B->nsrc * B->nblk * B->R * 4 + 2.0 * B->R * B->d * 4;
    ProfScope prof(VTC_PROF_TOPK, work, stream);
    const int na = cdiv(A.R, RK_OW), nb = B ? cdiv(B->R, RK_OW) : 0;
    auto kernel = npl_a == 4 ? recall_rank_kernel<4, 4> : npl_a == 3 ? recall_rank_kernel<3, 3> : npl_b == 3 ? recall_rank_kernel<2, 3> : recall_rank_kernel<2, 2>;
    hipLaunchKernelGGL(kernel, dim3(na + nb), dim3(256), 0, stream, A, Bv, na);
  }
  {
    ProfScope prof(VTC_PROF_TOPK, 0.0, stream);
    const int ga = std::min(A.R, 1024), gb = B ? std::min(B->R, 1024) : 0;
    hipLaunchKernelGGL(recall_rank_finish_kernel, dim3(ga + gb), dim3(64 * RK_FW), 0, stream, A, Bv, ga);
  }
}

// R@K hit counters of BOTH directions of n paired rows (a_i <-> b_i) without the sorted lists: prologue, ONE distance GEMM, ONE
// rank launch (+ the fallback launch, normally empty).  hits_b_from_a[j] += #{ i : rank of a_i among the a's for query b_i < k_j }
// (= RecallAtK.compute(a, b)), hits_a_from_b the transposed direction (= compute(b, a)).
int recall_bidir_impl(const float *a, const float *b, int n, int d, const KList &kl, unsigned long long *hits_b_from_a,
                      unsigned long long *hits_a_from_b, const Sweep2Ws &s, hipStream_t stream) {
  sweep_prologue(s, b, n, a, n, d, true, stream, s.flags, s.flags2);
  VTC_LAUNCH_CHECK("l2_recall prologue");
  const int mode = recall_mode(kl.kmax, n);
  GemmEpi e;
  e.mode = mode; e.out_dtype = VTC_F32; e.rown = s.qn; e.coln = s.gn;
  e.rowk = s.rowk; e.colk = s.colk; e.nblk_c = s.nblk_c; e.nblk_r = s.nblk_r;
  if (int rc = launch_gemm(s.qb, s.gb, nullptr, nullptr, n, n, d, VTC_BF16, e, stream)) return rc;
  const RecallArgs r1 = recall_args(s, b, a, n, n, d, 0, kl, hits_b_from_a);
  RecallArgs r2 = recall_args(s, a, b, n, n, d, 0, kl, hits_a_from_b);      // the column direction: the other side's planes, statistics and scratch
  r2.keys = s.colk; r2.nblk = s.nblk_r; r2.bw = RB2;
  r2.own_norm = s.gn; r2.own_st = s.gst; r2.other_max = s.qmax;
  r2.flags = s.flags2; r2.work = (int *)s.cand2; r2.part = s.cand2_n;
  launch_recall(r1, l2min_row_planes(mode), &r2, l2min_col_planes(mode), stream);
  VTC_LAUNCH_CHECK("l2_recall_bidir");
  return 0;
}
}  // namespace

// ---- the sharded exchange of sweep_topk.hip with the recall-only finish (round 5): hit counters instead of sorted lists -------------
extern "C" int vtc_l2_recall_planes(const int *k_vals, int nk, int n_total) {
  int kmax = 0;                                                // (a size query: no validation, the launches do that)
  for (int i = 0; k_vals && i < nk; ++i) kmax = std::max(kmax, k_vals[i]);
  return l2min_col_planes(recall_mode(kmax, n_total));       // (the planes that travel: the column direction's)
}

extern "C" int vtc_l2_recall_shard_supported(int n_total, int n_local, int d) {
  return d > 0 && d % 64 == 0 && n_local >= 1 && n_local <= n_total && exact2_enabled(n_total, n_local, 1);
}

extern "C" int vtc_l2_recall_shard_rows(const float *a_all, const float *b_local, int n_total, int n_local, int row_base, int d,
                                        const int *k_vals, int nk, long long *hits_b_from_a, unsigned *col_planes, int nblk_pad, void *ws,
                                        size_t ws_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(a_all && b_local && k_vals && hits_b_from_a && col_planes && ws, "l2_recall_shard_rows: null argument");
  VTC_CHECK(vtc_l2_recall_shard_supported(n_total, n_local, d), "l2_recall_shard_rows: unsupported shape (n_total=%d n_local=%d d=%d)", n_total, n_local, d);
  VTC_CHECK(row_base >= 0 && row_base + n_local <= n_total, "l2_recall_shard_rows: rows [%d, %d) outside [0, %d)", row_base, row_base + n_local, n_total);
  KList kl;
  if (int rc = read_k(kl, "l2_recall_shard_rows", k_vals, nk, n_total)) return rc;
  Sweep2Ws s = plan2((char *)ws, n_total, n_local, d, false);
  VTC_CHECK(nblk_pad >= s.nblk_r, "l2_recall_shard_rows: nblk_pad=%d < %d row blocks", nblk_pad, s.nblk_r);
  VTC_CHECK(ws_bytes >= vtc_l2_sweep_shard_workspace_bytes(n_total, n_local, d), "l2_recall_shard_rows: workspace too small");
  sweep_prologue(s, b_local, n_local, a_all, n_total, d, true, stream, s.flags);
  VTC_LAUNCH_CHECK("l2_recall_shard_rows prologue");
  const int mode = recall_mode(kl.kmax, n_total);
  GemmEpi e;
  e.mode = mode; e.out_dtype = VTC_F32; e.rown = s.qn; e.coln = s.gn;
  e.rowk = s.rowk; e.colk = col_planes; e.nblk_c = s.nblk_c; e.nblk_r = nblk_pad;
  fill_absent_row_blocks(col_planes, l2min_col_planes(mode), nblk_pad, s.nblk_r, n_total, stream);
  if (int rc = launch_gemm(s.qb, s.gb, nullptr, nullptr, n_local, n_total, d, VTC_BF16, e, stream)) return rc;
  const RecallArgs r = recall_args(s, b_local, a_all, n_local, n_total, d, row_base, kl, (unsigned long long *)hits_b_from_a);
  launch_recall(r, l2min_row_planes(mode), nullptr, 0, stream);
  VTC_LAUNCH_CHECK("l2_recall_shard_rows");
  return 0;
}

extern "C" int vtc_l2_recall_shard_cols(const float *b_all, const float *a_local, int n_total, int n_local, int row_base, int d,
                                        const int *k_vals, int nk, const unsigned *planes, int n_src, int nblk_pad, const int *src_bounds,
                                        long long *hits_a_from_b, void *ws, size_t ws_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(b_all && a_local && k_vals && planes && src_bounds && hits_a_from_b && ws, "l2_recall_shard_cols: null argument");
  VTC_CHECK(vtc_l2_recall_shard_supported(n_total, n_local, d) && n_src >= 1 && nblk_pad >= 1,
            "l2_recall_shard_cols: unsupported shape (n_total=%d n_local=%d d=%d n_src=%d)", n_total, n_local, d, n_src);
  VTC_CHECK(row_base >= 0 && row_base + n_local <= n_total, "l2_recall_shard_cols: rows [%d, %d) outside [0, %d)", row_base, row_base + n_local, n_total);
  KList kl;
  if (int rc = read_k(kl, "l2_recall_shard_cols", k_vals, nk, n_total)) return rc;
  VTC_CHECK(ws_bytes >= vtc_l2_sweep_shard_workspace_bytes(n_total, n_local, d), "l2_recall_shard_cols: workspace too small");
  // owners = a_local (this rank's columns of every source's GEMM), the other side = b_all: the plan's areas fit as they are
  Sweep2Ws s = plan2((char *)ws, n_total, n_local, d, false);
  sweep_prologue(s, a_local, n_local, b_all, n_total, d, false, stream, s.flags);
  RecallArgs r = recall_args(s, a_local, b_all, n_local, n_total, d, row_base, kl, (unsigned long long *)hits_a_from_b);
  r.keys = planes; r.nblk = nblk_pad; r.bw = RB2; r.nsrc = n_src; r.bounds = src_bounds;      // every source's planes of this rank's columns
  launch_recall(r, l2min_col_planes(recall_mode(kl.kmax, n_total)), nullptr, 0, stream);
  VTC_LAUNCH_CHECK("l2_recall_shard_cols");
  return 0;
}

extern "C" int vtc_l2_recall_bidir_supported(int n, int d) { return (n >= 1024 && d > 0 && d % 64 == 0) ? 1 : 0; }
extern "C" size_t vtc_l2_recall_bidir_workspace_bytes(int n, int d) { return plan2(nullptr, n, n, d, true).total; }
extern "C" int vtc_l2_recall_bidir(const float *a, const float *b, int n, int d, const int *k_vals, int nk, long long *hits_b_from_a,
                                   long long *hits_a_from_b, void *ws, size_t ws_bytes, void *stream) {
  VTC_CHECK(a && b && hits_b_from_a && hits_a_from_b && k_vals, "l2_recall_bidir: null argument");
  VTC_CHECK(vtc_l2_recall_bidir_supported(n, d), "l2_recall_bidir: n=%d must be >= 1024 and d=%d a multiple of 64 (else: vtc_l2_topk + vtc_recall_hits)", n, d);
  KList kl;
  if (int rc = read_k(kl, "l2_recall_bidir", k_vals, nk, n)) return rc;
  Sweep2Ws s = plan2((char *)ws, n, n, d, true);
  VTC_CHECK(ws && ws_bytes >= s.total, "l2_recall_bidir: workspace too small (%zu < %zu)", ws_bytes, s.total);
  return recall_bidir_impl(a, b, n, d, kl, (unsigned long long *)hits_b_from_a, (unsigned long long *)hits_a_from_b, s, (hipStream_t)stream);
}
