// search_q8.hip -- the query-time search over a gallery stored as 8-BIT CODES, one fp32 scale a row (include/vtc_hip.h, "a q8 row":
// d signed codes, the scale at byte d, 12 bytes of padding; the stored value of a column is fl32(scale * code)).  Nothing of the search
// is defined again here: the scan, the mark pass, the pair distances, the merges and the driver are search.hip's (search_scan.h),
// instantiated with G = q8_t, whose row loader (sweep_common.h: q8_row, q8_scale, row_piece(Q8Piece)) hands wave_dist64_core the four
// fp32 products of a piece where the fp32 scan loads four floats -- the same statements in the same order after that, so every output
// has the bits of the fp32 entries over the gallery of the stored values.  This file holds the q8 entries and, through them, the q8
// instantiations of the non-SET kernels (the SET ones are search_sets_q8.hip's, the range passes range_q8.hip's), and the quantiser.
#include "search_scan.h"

namespace {
using namespace vtcsweep;

// fp32 rows -> q8 rows, a wave per row, by the rule of include/vtc_hip.h: m = max |x_k|; t = fl32(m / 127); the scale s is t rounded
// UP to 16 significant bits (so that s * code is exact in fp32); s = 1 for a row of zeros; code_k = clamp(rint(fl32(x_k / s)), -127, 127),
// ties to even.  Both divisions are correctly rounded (__fdiv_rn).  A row with a NaN / inf gets s = NaN and codes of 0 and sets bit 1
// of `nonfinite`.  The row is read twice, the second time out of the cache; a lane writes its 4 codes as one word, lane 0 the scale,
// lanes 1 .. 3 the zero padding.
__global__ __launch_bounds__(256) void quantize_rows_q8_kernel(const float *__restrict__ x, int n, int d, q8_t *__restrict__ rows_out,
                                                               int *__restrict__ nonfinite) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;                                    // wave-uniform
  const float *xr = x + (size_t)row * d;
  float m = 0.0f;
  bool bad = false;
  for (int c = lane * 4; c < d; c += 256) {
    const float4 v = *reinterpret_cast<const float4 *>(xr + c);
    const float a = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));      // fmaxf drops a NaN: asked below
    bad |= !(fabsf(v.x) < INFINITY) || !(fabsf(v.y) < INFINITY) || !(fabsf(v.z) < INFINITY) || !(fabsf(v.w) < INFINITY);
    m = fmaxf(m, a);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  bad = __ballot(bad) != 0;
  float s = 1.0f;
  if (bad) {
    s = __uint_as_float(0x7fc00000u);
  } else if (m != 0.0f) {
    s = __uint_as_float((__float_as_uint(__fdiv_rn(m, 127.0f)) + 0xffu) & ~0xffu);
  }
  q8_t *out = rows_out + (size_t)row * (size_t)(d + Q8_TAIL);
  for (int c = lane * 4; c < d; c += 256) {
    unsigned word = 0;
    if (!bad) {
      const float4 v = *reinterpret_cast<const float4 *>(xr + c);
      const float q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int code = (int)fminf(fmaxf(rintf(__fdiv_rn(q[k], s)), -127.0f), 127.0f);
        word |= ((unsigned)code & 0xffu) << (8 * k);
      }
    }
    *reinterpret_cast<unsigned *>(out + c) = word;
  }
  if (lane == 0) *reinterpret_cast<float *>(out + d) = s;
  else if (lane < 4) *reinterpret_cast<unsigned *>(out + d + 4 * lane) = 0u;
  if (bad && nonfinite && lane == 0) atomicOr(nonfinite, 1);
}
}  // namespace

extern "C" size_t vtc_q8_row_bytes(int d) { return d >= 64 && d <= SEARCH_MAX_D && d % 64 == 0 ? (size_t)d + Q8_TAIL : 0; }

extern "C" int vtc_quantize_rows_q8(const float *x, int n, int d, void *rows_out, int *nonfinite, void *stream) {
  VTC_CHECK(x && rows_out, "quantize_rows_q8: null argument");
  VTC_CHECK(n >= 1, "quantize_rows_q8: n=%d must be at least 1", n);
  VTC_CHECK(d >= 64 && d <= SEARCH_MAX_D && d % 64 == 0, "quantize_rows_q8: d=%d must be a multiple of 64 in [64, %d]", d, SEARCH_MAX_D);
  VTC_CHECK(((uintptr_t)x | (uintptr_t)rows_out) % 16 == 0, "quantize_rows_q8: x and rows_out must be 16-byte aligned");
  hipLaunchKernelGGL(quantize_rows_q8_kernel, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, x, n, d, static_cast<q8_t *>(rows_out), nonfinite);
  VTC_LAUNCH_CHECK("quantize_rows_q8");
  return 0;
}

// One entry for the six scan modes: which of live, groups, exclude, the cursor and the ban bitmap are given chooses the scan
// (launch_scan_of), by check_search_call's rules.
extern "C" int vtc_l2_search_q8(const void *gallery, const float *queries, const uint32_t *live, const int32_t *groups, int n_groups,
                                const uint32_t *ban, const int64_t *exclude, const double *after_d, const int64_t *after_i, int ng, int nq, int d,
                                int depth, int64_t id_base, int64_t *ids, int32_t *out_groups, float *dists, int *nonfinite, void *ws,
                                size_t ws_bytes, void *stream) {
  VTC_CHECK(!ban || (groups && after_d), "l2_search_q8: ban (the page scan) needs groups and a cursor");
  return search_entry_of<q8_t>("l2_search_q8", {gallery, false, queries, live, groups, after_d, after_i, exclude, ban, n_groups, ng, nq, d, depth, id_base,
                                                ids, out_groups, dists, nonfinite, ws, ws_bytes, stream, true});
}

extern "C" int vtc_l2_group_mark_before_q8(const void *gallery, const float *queries, const uint32_t *live, const int32_t *groups, int n_groups,
                                           const double *after_d, const int64_t *after_i, int ng, int nq, int d, int64_t id_base, uint32_t *ban,
                                           void *stream) {
  return mark_before<q8_t>(gallery, queries, live, groups, n_groups, after_d, after_i, ng, nq, d, id_base, ban, stream);
}

extern "C" int vtc_l2_pair_dists64_q8(const void *gallery, const float *queries, const int64_t *rows, int ng, int nq, int d, int64_t id_base,
                                      double *out, void *stream) {
  return pair_dists64<q8_t>(gallery, queries, rows, ng, nq, d, id_base, out, stream);
}
