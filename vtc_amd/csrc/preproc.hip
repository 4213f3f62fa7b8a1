// preproc.hip -- decoded frames -> the tower's uint8 pixels: Resize(size, BICUBIC) + CenterCrop(size) of CLIP_TRANSFORM
// (dataset_loaders/dataset_loaders.py:40-49, video_retrieval_videodatasets.py:21-29), bit for bit what Pillow's 8-bit resampler and
// torchvision's size / crop arithmetic give.  ToTensor + Normalize, the other half of that transform, are the VTC_U8 path of embed.hip.
//   vtc_resize_plan_bytes / vtc_resize_plan   host: the taps of the cropped output columns and rows, coefficients from doubles
//   vtc_resize_crop_u8                        one launch: horizontal pass into LDS, vertical pass out of it
#include "common.h"

#include <math.h>
#include <string.h>

namespace {

constexpr int kPrecisionBits = 22;               // Pillow's PRECISION_BITS for 8-bit images (32 - 8 - 2)
constexpr int kMagic = 0x31505256;               // "VRP1"
constexpr int kHeaderWords = 16;
constexpr int kMaxEdge = 8192, kMaxSize = 1024;  // source edges / output edge (include/vtc_hip.h)
constexpr int kThreads = 256, kThreadsLong = 1024;   // workgroup sizes: short / long vertical supports (vtc_resize_crop_u8)
constexpr int kLdsTwoBlocks = 72 * 1024;         // staging that leaves room for two workgroups on a CU's 160 KiB
constexpr int kLdsOneBlock = 144 * 1024;

struct Geometry {
  int out_w, out_h, left, top, kx, ky;
};

// torchvision CenterCrop: int(round((n_out - size) / 2.0)), Python's round (ties to even)
int crop_offset(int n_out, int size) {
  const int d = n_out - size;
  return (d & 1) ? (d / 2 + ((d / 2) & 1)) : d / 2;
}

int tap_count(int n_in, int n_out) {
  if (n_in == n_out) return 1;
  double fs = (double)n_in / n_out;
  if (fs < 1.0) fs = 1.0;
  return (int)ceil(2.0 * fs) * 2 + 1;
}

bool geometry(int in_h, int in_w, int size, Geometry *g) {
  if (size <= 0 || size % 16 || size > kMaxSize || in_h < 1 || in_w < 1 || in_h > kMaxEdge || in_w > kMaxEdge) return false;
  // torchvision Resize(int): the shorter edge becomes size, the longer trunc(size * long / short) (the double quotient of the exact product)
  if (in_w <= in_h) {
    g->out_w = size;
    g->out_h = (int)((double)((long long)size * in_h) / (double)in_w);
  } else {
    g->out_h = size;
    g->out_w = (int)((double)((long long)size * in_w) / (double)in_h);
  }
  g->left = crop_offset(g->out_w, size);
  g->top = crop_offset(g->out_h, size);
  g->kx = tap_count(in_w, g->out_w);
  g->ky = tap_count(in_h, g->out_h);
  return true;
}

size_t plan_words(const Geometry &g, int size) { return kHeaderWords + (size_t)size * (2 + g.kx) + (size_t)size * (2 + g.ky); }

// Output rows per workgroup: the horizontally resampled source rows of a band stay in LDS, 3 * size bytes each.  A band of R rows needs
// at most ceil((R - 1) * scale) + ky + 1 of them (first and last window are (R - 1) * scale apart, a window is at most ky wide).
int staged_rows(int in_h, int out_h, int ky, int band) { return (int)(((long long)(band - 1) * in_h + out_h - 1) / out_h) + ky + 1; }
int choose_band(int in_h, int size, const Geometry &g) {
  for (int band = 16; band >= 1; band >>= 1)
    if ((size_t)staged_rows(in_h, g.out_h, g.ky, band) * 3 * size <= (size_t)(band > 1 ? kLdsTwoBlocks : kLdsOneBlock)) return band;
  return 0;
}

#pragma clang fp contract(off)
double bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// `size` records of (first, count, coef[ksize]) for the output indices lo .. lo + size - 1 (Pillow's precompute_coeffs + normalize_coeffs_8bpc)
void axis_plan(int n_in, int n_out, int lo, int size, int ksize, int32_t *rec, double *w) {
  for (int i = 0; i < size; ++i, rec += 2 + ksize) {
    if (n_in == n_out) {   // Pillow skips a pass that changes nothing
      rec[0] = lo + i; rec[1] = 1; rec[2] = 1 << kPrecisionBits;
      continue;
    }
    const double scale = (double)n_in / n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs, ss = 1.0 / fs;
    const double center = (lo + i + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > n_in) xmax = n_in;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      w[x] = bicubic((x + xmin - center + 0.5) * ss);
      ww += w[x];
    }
    rec[0] = xmin; rec[1] = xmax;
    for (int x = 0; x < ksize; ++x) {
      if (x >= xmax) { rec[2 + x] = 0; continue; }
      const double v = ww != 0.0 ? w[x] / ww : w[x];
      rec[2 + x] = v < 0 ? (int)(-0.5 + v * (1 << kPrecisionBits)) : (int)(0.5 + v * (1 << kPrecisionBits));
    }
  }
}

struct ResizeArgs {
  const unsigned char *frames;
  const int32_t *plan;
  unsigned char *out;
  int in_h, in_w, layout, size, band, bands, lds_rows;
  Geometry g;
};

// clamp(v >> 22, 0, 255), with the clamp in front of the shift (the same value: the shift is monotonic).  Written shift-first, hipcc
// pairs two of them into v_ashr_pk_u8_i32, and the word it then ORs the other bytes into came back from the MI355X with a bit set
// above the two packed bytes (every third byte of a 16-byte store off by 64).
__device__ __forceinline__ int clamp_u8(int v) { return min(max(v, 0), (256 << kPrecisionBits) - 1) >> kPrecisionBits; }

// One workgroup = one frame x one band of output rows, all three channels.  Pass 1 resamples the source rows in the band's vertical
// support along x into LDS ([row][channel][x], uint8: Pillow rounds the intermediate image); pass 2 resamples those along y, 16 output
// pixels per thread, one 16-byte store each.  Every index taken from the plan is clamped to the arrays it addresses.
__global__ __launch_bounds__(kThreadsLong) void resize_crop_kernel(const ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char stage[];
  const int32_t *hdr = a.plan;
  if (hdr[0] != kMagic || hdr[1] != a.in_h || hdr[2] != a.in_w || hdr[3] != a.size || hdr[4] != a.g.out_w || hdr[5] != a.g.out_h ||
      hdr[6] != a.g.left || hdr[7] != a.g.top || hdr[8] != a.g.kx || hdr[9] != a.g.ky)
    return;                                          // a plan made for other arguments: nothing is read or written
  const int size = a.size, kx = a.g.kx, ky = a.g.ky;
  const int32_t *cols = a.plan + kHeaderWords, *rows = cols + (size_t)size * (2 + kx);
  const size_t frame = blockIdx.x / a.bands;
  const int y0 = (blockIdx.x % a.bands) * a.band, y1 = min(y0 + a.band, size);
  const unsigned char *src = a.frames + frame * ((size_t)a.in_h * a.in_w * 3);

  const int32_t *rlast = rows + (size_t)(y1 - 1) * (2 + ky);
  const int ymin = min(max(rows[(size_t)y0 * (2 + ky)], 0), a.in_h - 1);
  const int nrows = min(min(max(rlast[0] + rlast[1] - ymin, 0), a.lds_rows), a.in_h - ymin);

  // pass 1: (source row, output column) per thread, the three channels together
  const size_t chan = a.layout ? (size_t)a.in_h * a.in_w : 1, pix = a.layout ? 1 : 3;
  for (int idx = threadIdx.x; idx < nrows * size; idx += blockDim.x) {
    const int r = idx / size, x = idx - r * size;
    const int32_t *rec = cols + (size_t)x * (2 + kx);
    const int first = min(max(rec[0], 0), a.in_w - 1), cnt = min(min(rec[1], kx), a.in_w - first);
    const unsigned char *p = src + ((size_t)(ymin + r) * a.in_w + first) * pix;
    int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < cnt; ++t, p += pix) {
      const int k = rec[2 + t];
      s0 += p[0] * k;
      s1 += p[chan] * k;
      s2 += p[2 * chan] * k;
    }
    unsigned char *d = stage + (size_t)r * 3 * size + x;
    d[0] = (unsigned char)clamp_u8(s0);
    d[size] = (unsigned char)clamp_u8(s1);
    d[2 * size] = (unsigned char)clamp_u8(s2);
  }
  __syncthreads();

  // pass 2: (output row, channel, 16 columns) per thread
  const int groups = size / 16;
  for (int idx = threadIdx.x; idx < (y1 - y0) * 3 * groups; idx += blockDim.x) {
    const int gx = idx % groups, c = (idx / groups) % 3, y = y0 + idx / (3 * groups);
    const int32_t *rec = rows + (size_t)y * (2 + ky);
    const int rel = min(max(rec[0] - ymin, 0), nrows), cnt = min(min(rec[1], ky), nrows - rel);
    int acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 1 << (kPrecisionBits - 1);
    const unsigned char *s = stage + ((size_t)rel * 3 + c) * size + gx * 16;
    for (int t = 0; t < cnt; ++t, s += 3 * size) {
      const int k = rec[2 + t];
      const uint4 v = *reinterpret_cast<const uint4 *>(s);
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[j] += (int)((w[j >> 2] >> (8 * (j & 3))) & 255u) * k;
    }
    unsigned o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      o[q] = (unsigned)clamp_u8(acc[4 * q]) | ((unsigned)clamp_u8(acc[4 * q + 1]) << 8) | ((unsigned)clamp_u8(acc[4 * q + 2]) << 16) |
             ((unsigned)clamp_u8(acc[4 * q + 3]) << 24);
    unsigned char *dst = a.out + ((frame * 3 + c) * size + y) * (size_t)size + gx * 16;
    *reinterpret_cast<uint4 *>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

PerDeviceOnce g_resize_lds;

}  // namespace

extern "C" size_t vtc_resize_plan_bytes(int in_h, int in_w, int size) {
  Geometry g;
  if (!geometry(in_h, in_w, size, &g) || !choose_band(in_h, size, g)) return 0;
  return plan_words(g, size) * sizeof(int32_t);
}

extern "C" int vtc_resize_plan(int in_h, int in_w, int size, void *plan_host, size_t bytes) {
  Geometry g;
  VTC_CHECK(size > 0 && size % 16 == 0 && size <= kMaxSize, "resize_plan: size=%d must be a positive multiple of 16, at most %d", size, kMaxSize);
  VTC_CHECK(in_h >= 1 && in_w >= 1 && in_h <= kMaxEdge && in_w <= kMaxEdge, "resize_plan: source %d x %d: edges must lie in [1, %d]", in_h,
            in_w, kMaxEdge);
  VTC_CHECK(geometry(in_h, in_w, size, &g) && choose_band(in_h, size, g), "resize_plan: %d x %d -> %d: one output row's support does not fit the LDS",
            in_h, in_w, size);
  const size_t need = plan_words(g, size) * sizeof(int32_t);
  VTC_CHECK(plan_host && bytes >= need, "resize_plan: plan buffer of %zu bytes, %zu needed", plan_host ? bytes : (size_t)0, need);
  int32_t *p = (int32_t *)plan_host;
  memset(p, 0, kHeaderWords * sizeof(int32_t));
  p[0] = kMagic; p[1] = in_h; p[2] = in_w; p[3] = size; p[4] = g.out_w; p[5] = g.out_h; p[6] = g.left; p[7] = g.top; p[8] = g.kx; p[9] = g.ky;
  double w[2 * (2 * kMaxEdge / 16 + 1) + 2];        // the most taps an axis can have: size >= 16, scale <= kMaxEdge / 16
  axis_plan(in_w, g.out_w, g.left, size, g.kx, p + kHeaderWords, w);
  axis_plan(in_h, g.out_h, g.top, size, g.ky, p + kHeaderWords + (size_t)size * (2 + g.kx), w);
  return 0;
}

extern "C" int vtc_resize_crop_u8(const unsigned char *frames, int n, int in_h, int in_w, int layout, const void *plan_dev, int size,
                                  unsigned char *out, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ResizeArgs a;
  VTC_CHECK(size > 0 && size % 16 == 0 && size <= kMaxSize, "resize_crop_u8: size=%d must be a positive multiple of 16, at most %d", size, kMaxSize);
  VTC_CHECK(in_h >= 1 && in_w >= 1 && in_h <= kMaxEdge && in_w <= kMaxEdge, "resize_crop_u8: source %d x %d: edges must lie in [1, %d]", in_h,
            in_w, kMaxEdge);
  VTC_CHECK(layout == 0 || layout == 1, "resize_crop_u8: layout=%d (0: [n, h, w, 3], 1: [n, 3, h, w])", layout);
  VTC_CHECK(n >= 1, "resize_crop_u8: n=%d", n);
  VTC_CHECK(frames && plan_dev && out, "resize_crop_u8: null pointer");
  VTC_CHECK(((uintptr_t)out & 15) == 0 && ((uintptr_t)plan_dev & 3) == 0, "resize_crop_u8: out must be 16-byte aligned, the plan 4-byte aligned");
  VTC_CHECK(geometry(in_h, in_w, size, &a.g), "resize_crop_u8: bad geometry");
  a.band = choose_band(in_h, size, a.g);
  VTC_CHECK(a.band, "resize_crop_u8: %d x %d -> %d: one output row's support does not fit the LDS", in_h, in_w, size);
  a.bands = cdiv(size, a.band);
  VTC_CHECK((long long)n * a.bands <= 0x7fffffffll, "resize_crop_u8: n=%d frames x %d bands exceed the grid", n, a.bands);
  a.frames = frames; a.plan = (const int32_t *)plan_dev; a.out = out;
  a.in_h = in_h; a.in_w = in_w; a.layout = layout; a.size = size;
  a.lds_rows = staged_rows(in_h, a.g.out_h, a.g.ky, a.band);
  const size_t lds = align_up((size_t)a.lds_rows * 3 * size, 16);
  if (ensure_dynamic_lds(g_resize_lds, (const void *)resize_crop_kernel, kLdsOneBlock, "resize_crop_u8")) return 1;
  // bytes that must move: the crop window of the source (with its taps' margin) once, the output once
  const double win_w = fmin((double)in_w, (double)size * in_w / a.g.out_w + a.g.kx), win_h = fmin((double)in_h, (double)size * in_h / a.g.out_h + a.g.ky);
  ProfScope prof(VTC_PROF_EMBED, (double)n * 3.0 * (win_w * win_h + (double)size * size), stream);
  // A long support's staging leaves room for two or three workgroups on a CU: those run 16 waves each instead of 4, so that the CU stays
  // full of waves (measured at size 224: 720 x 1280 5.99 -> 5.36 us per frame, 1080 x 1920 15.6 -> 15.4; profiles/preproc.md).
  const int threads = lds > 40 * 1024 ? kThreadsLong : kThreads;
  hipLaunchKernelGGL(resize_crop_kernel, dim3(n * a.bands), dim3(threads), lds, stream, a);
  VTC_LAUNCH_CHECK("resize_crop_u8");
  return 0;
}
