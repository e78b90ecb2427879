// Input pipeline (reference dataset.py:19-26 load_image):
//   img = tf.image.resize(decode_jpeg(file, channels=3), (S, S))   # bilinear
//   img = mobilenet_v2.preprocess_input(img)                       # x/127.5 - 1
// for a whole batch of decoded, ragged-size uint8 RGB images in ONE launch,
// writing the NHWC fp32 / bf16 model input directly.
//
// TF2 tf.image.resize (ResizeBilinear, half_pixel_centers=True,
// align_corners=False, antialias=False), per output coordinate i of an axis:
//   scale = float(in_size) / float(out_size)
//   in    = (float(i) + 0.5f) * scale - 0.5f
//   lower = max(int(floor(in)), 0), upper = min(int(ceil(in)), in_size - 1)
//   lerp  = in - floor(in)
//   top = tl + (tr - tl) * xlerp; bottom = bl + (br - bl) * xlerp
//   out = top + (bottom - top) * ylerp
// in fp32 with every multiply and add rounded separately (no FMA
// contraction: the pragma below), so the result is bit-identical to the
// restatement in oracle/image_ref.py. Then out / div - sub (an IEEE divide,
// as the Keras preprocessing's `x /= 127.5`, not a reciprocal multiply).
//
// One 256-thread block per (image, output row): the two source rows the row
// interpolates between are staged in LDS with coalesced dword loads (the
// decoded rows are byte-packed, 3 B per pixel, so a row starts at any byte;
// the staging window starts at the dword below), then each thread produces
// output pixels from LDS. Rows wider than the LDS window read global memory
// directly. HBM-bound: the output (12 B / pixel fp32) dominates.
#include "common.h"

namespace fpnmt {
namespace {

constexpr int IMG_THREADS = 256;
constexpr int IMG_LDS_MAX = 64 * 1024;  // dynamic LDS per block for the two staged rows

struct Axis {
  int lo, hi;
  float lerp;
};

__device__ __forceinline__ Axis axis_weights(int i, float scale, int in_size) {
#pragma clang fp contract(off)
  const float in = ((float)i + 0.5f) * scale - 0.5f;
  const float f = floorf(in);
  Axis a;
  a.lo = max((int)f, 0);
  a.hi = min((int)ceilf(in), in_size - 1);
  a.lerp = in - f;
  return a;
}

__device__ __forceinline__ float lerp2(float tl, float tr, float bl, float br, float xl, float yl) {
#pragma clang fp contract(off)
  const float top = tl + (tr - tl) * xl;
  const float bottom = bl + (br - bl) * xl;
  return top + (bottom - top) * yl;
}

// bytes [start, start + len) of the packed buffer into LDS in 16-B pieces,
// from the 16-B boundary at or below `start` (the packed buffer is 16-B
// aligned); returns the byte shift of `start` inside the window
__device__ __forceinline__ int stage_row(uint32_t* lds, const uint8_t* px, long long px_bytes, long long start,
                                         int len) {
  const long long base = start & ~15LL;
  const int nq = (int)((start + len - base + 15) >> 4);
  const uint4* g = (const uint4*)(px + base);
  for (int i = threadIdx.x; i < nq; i += IMG_THREADS) {
    const long long b = base + 16LL * i;
    uint4 v;
    if (b + 15 < px_bytes) {
      v = g[i];
    } else {  // the buffer's last partial piece: byte loads
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      for (int k = 0; k < 16; ++k)
        if (b + k < px_bytes) w[k >> 2] |= (uint32_t)px[b + k] << (8 * (k & 3));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *(uint4*)(lds + 4 * i) = v;
  }
  return (int)(start - base);
}

// LDS words of one staged row window: the row's bytes + up to 15 leading
// bytes, rounded up to whole 16-B pieces
__host__ __device__ __forceinline__ int row_window_words(int row_bytes) { return ((row_bytes + 30) / 16) * 4; }

// One 256-thread block per (image, RB consecutive output rows): the 2*RB
// source rows are staged in LDS with coalesced dword loads, then the block
// writes the RB output rows as runs of 4 consecutive values (one 16-B fp32 /
// 8-B bf16 store per thread per run; a value's pixel and channel are v / 3,
// v % 3), so a block issues ~170 wide stores per row instead of 672 scalar
// ones and a grid of 56 blocks per 224-row image instead of 224.
template <typename T, int RB, bool USE_LDS>
__global__ __launch_bounds__(IMG_THREADS) void resize_normalize_kernel(const fpnmt_image_item* __restrict__ items,
                                                                        const uint8_t* __restrict__ px,
                                                                        long long px_bytes, int row_words,
                                                                        int out_h, int out_w, float div, float sub,
                                                                        T* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ uint32_t lds[];
  const int y0 = blockIdx.x * RB, img = blockIdx.y;
  const fpnmt_image_item it = items[img];
  const int rv = out_w * 3;  // values per output row
  if (it.h <= 0 || it.w <= 0) {  // the host loader rejects empty images; keep the output defined
    for (int r = 0; r < RB && y0 + r < out_h; ++r) {
      T* orow = out + ((long long)img * out_h + y0 + r) * rv;
      for (int x = threadIdx.x; x < rv; x += IMG_THREADS) orow[x] = from_f32<T>(0.f);
    }
    return;
  }
  const int rb = it.w * 3;
  const float yscale = (float)it.h / (float)out_h, xscale = (float)it.w / (float)out_w;
  const uint8_t* top[RB];
  const uint8_t* bot[RB];
  float ylerp[RB];
  const bool staged = USE_LDS && row_window_words(rb) <= row_words;
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    const Axis ya = axis_weights(min(y0 + r, out_h - 1), yscale, it.h);
    ylerp[r] = ya.lerp;
    if (staged) {
      // (the item's row fits the window sized for max_w; a wider row than
      // the caller declared reads global memory instead of overrunning LDS)
      uint32_t* l0 = lds + (2 * r) * row_words;
      uint32_t* l1 = lds + (2 * r + 1) * row_words;
      const int s0 = stage_row(l0, px, px_bytes, it.offset + (long long)ya.lo * rb, rb);
      const int s1 = stage_row(l1, px, px_bytes, it.offset + (long long)ya.hi * rb, rb);
      top[r] = (const uint8_t*)l0 + s0;
      bot[r] = (const uint8_t*)l1 + s1;
    } else {
      top[r] = px + it.offset + (long long)ya.lo * rb;
      bot[r] = px + it.offset + (long long)ya.hi * rb;
    }
  }
  if (staged) __syncthreads();
  auto value = [&](int r, int v) {
    const int x = v / 3, ch = v - 3 * x;
    const Axis xa = axis_weights(x, xscale, it.w);
    const int a = xa.lo * 3 + ch, b = xa.hi * 3 + ch;
    const float f = lerp2((float)top[r][a], (float)top[r][b], (float)bot[r][a], (float)bot[r][b], xa.lerp, ylerp[r]);
    return f / div - sub;
  };
  const bool vec = (rv & 3) == 0;  // every row starts 4-value aligned
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    if (y0 + r >= out_h) break;
    T* orow = out + ((long long)img * out_h + y0 + r) * rv;
    if (vec) {
      typedef __attribute__((ext_vector_type(4))) T T4;
      for (int q = threadIdx.x; q < (rv >> 2); q += IMG_THREADS) {
        T4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = from_f32<T>(value(r, 4 * q + j));
        *(T4*)(orow + 4 * q) = o;
      }
    } else {
      for (int v = threadIdx.x; v < rv; v += IMG_THREADS) orow[v] = from_f32<T>(value(r, v));
    }
  }
}

template <typename T>
void resize_launch(const fpnmt_image_item* items, int n, const uint8_t* px, long long px_bytes, int max_w, int out_h,
                   int out_w, float div, float sub, void* out, hipStream_t s) {
  constexpr int RB = 4;
  const int row_words = row_window_words(max_w * 3);
  const size_t lds4 = 2ull * RB * row_words * 4, lds1 = 2ull * row_words * 4;
  const bool aligned = ((uintptr_t)px & 15) == 0;  // the staging reads 16-B pieces of the packed buffer
  if (aligned && lds4 <= (size_t)IMG_LDS_MAX)
    resize_normalize_kernel<T, RB, true><<<dim3(cdiv(out_h, RB), n), IMG_THREADS, lds4, s>>>(
        items, px, px_bytes, row_words, out_h, out_w, div, sub, (T*)out);
  else if (aligned && lds1 <= (size_t)IMG_LDS_MAX)
    resize_normalize_kernel<T, 1, true><<<dim3(out_h, n), IMG_THREADS, lds1, s>>>(items, px, px_bytes, row_words,
                                                                                   out_h, out_w, div, sub, (T*)out);
  else
    resize_normalize_kernel<T, 1, false><<<dim3(out_h, n), IMG_THREADS, 0, s>>>(items, px, px_bytes, 0, out_h, out_w,
                                                                                div, sub, (T*)out);
}

// ---- train-time augmentation (include/fpnmt.h: fpnmt_image_aug) ----------
// The same resize over a crop box of each image, optionally mirrored, then
// contrast / brightness / saturation on the resized fp32 value, then the
// normalisation. Every step is the individually rounded fp32 operation the
// header states, so the result equals the numpy restatement bit for bit, and
// a record with the full box, no flip and all factors 1.0f takes exactly the
// arithmetic of resize_normalize_kernel.

struct Box {
  int y0, x0, ch, cw;
};

// the record's box intersected with its image (the records are device data
// nobody validated on the way in); 64-bit so y0 + ch cannot wrap
__device__ __forceinline__ Box clamp_box(const fpnmt_image_item& it, const fpnmt_image_aug& a) {
  const long long ya = max((long long)a.y0, 0LL), yb = min((long long)a.y0 + a.ch, (long long)it.h);
  const long long xa = max((long long)a.x0, 0LL), xb = min((long long)a.x0 + a.cw, (long long)it.w);
  Box b;
  b.ch = (int)max(yb - ya, 0LL);
  b.cw = (int)max(xb - xa, 0LL);
  b.y0 = b.ch ? (int)ya : 0;
  b.x0 = b.cw ? (int)xa : 0;
  return b;
}

constexpr int STATS_CHUNKS = 32;  // row chunks per image: blocks of image_crop_stats_kernel

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// R, G, B byte sums of each image's box. One block per (image, chunk of box
// rows); a thread takes 16-B pieces of the row segment [x0*3, (x0+cw)*3) from
// the 16-B boundary below it (pieces of all the chunk's rows are dealt to the
// threads in one sequence, so narrow boxes keep the block busy). The channel
// of a byte is its position mod 3 within the segment: a piece is summed by
// its static byte position mod 3 into 32-bit partials, which the piece's
// phase then rotates onto the channels' 64-bit thread totals. One block
// reduction, one 64-bit integer atomicAdd per channel per block.
__global__ __launch_bounds__(IMG_THREADS) void image_crop_stats_kernel(const fpnmt_image_item* __restrict__ items,
                                                                        const fpnmt_image_aug* __restrict__ aug,
                                                                        const uint8_t* __restrict__ px,
                                                                        long long px_bytes, int aligned,
                                                                        unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long red[3][IMG_THREADS / 64];
  const int img = blockIdx.y;
  const fpnmt_image_item it = items[img];
  if (it.h <= 0 || it.w <= 0) return;
  const Box bx = clamp_box(it, aug[img]);
  if (bx.ch <= 0 || bx.cw <= 0) return;
  const int rows_per = (bx.ch + (int)gridDim.x - 1) / (int)gridDim.x;
  const int r0 = blockIdx.x * rows_per, r1 = min(r0 + rows_per, bx.ch);
  if (r0 >= r1) return;  // (block-uniform, like the returns above)
  const int rb = it.w * 3, bb = bx.cw * 3;
  const int np = (bb + 30) >> 4;  // 16-B pieces that can hold a segment starting at any byte
  const long long origin = it.offset + (long long)(bx.y0 + r0) * rb + (long long)bx.x0 * 3;
  unsigned long long acc0 = 0, acc1 = 0, acc2 = 0;
  int r = threadIdx.x / np, p = threadIdx.x - r * np;
  while (r < r1 - r0) {
    const long long start = origin + (long long)r * rb;
    const long long b = (start & ~15LL) + 16LL * p;
    const int d = (int)(b - start);  // >= -15: the segment's byte of the piece's byte 0
    if (d < bb) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (aligned && b + 15 < px_bytes) {
        const uint4 v = *(const uint4*)(px + b);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
      } else {  // the buffer's last partial piece (or an unaligned buffer): byte loads
        for (int k = 0; k < 16; ++k)
          if (b + k < px_bytes) w[k >> 2] |= (uint32_t)px[b + k] << (8 * (k & 3));
      }
      const int lo = max(-d, 0), hi = min(bb - d, 16);
      uint32_t t[3] = {0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 16; ++k)
        t[k % 3] += (k >= lo && k < hi) ? ((w[k >> 2] >> (8 * (k & 3))) & 255u) : 0u;
      const int ph = (d + 15) % 3;  // byte k of the piece is channel (ph + k) % 3
      acc0 += ph == 0 ? t[0] : ph == 1 ? t[2] : t[1];
      acc1 += ph == 0 ? t[1] : ph == 1 ? t[0] : t[2];
      acc2 += ph == 0 ? t[2] : ph == 1 ? t[1] : t[0];
    }
    p += IMG_THREADS;
    while (p >= np) p -= np, ++r;
  }
  acc0 = wave_sum_u64(acc0), acc1 = wave_sum_u64(acc1), acc2 = wave_sum_u64(acc2);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[0][wave] = acc0, red[1][wave] = acc1, red[2][wave] = acc2;
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long s = 0;
    for (int k = 0; k < IMG_THREADS / 64; ++k) s += red[threadIdx.x][k];
    atomicAdd(sums + 4LL * img + threadIdx.x, s);
  }
}

// the block-uniform colour parameters of one image
struct Colour {
  bool contrast, bright, sat;
  float m, cf, bf, sf;
};

__device__ __forceinline__ float clamp255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }

// contrast, then brightness, of one resized value
__device__ __forceinline__ float tone(float v, const Colour& c) {
#pragma clang fp contract(off)
  if (c.contrast) v = clamp255(c.m + (v - c.m) * c.cf);
  if (c.bright) v = clamp255(v * c.bf);
  return v;
}

// saturation of one pixel's three (toned) values
__device__ __forceinline__ void saturate(float* p, float sf) {
#pragma clang fp contract(off)
  const float g = 0.299f * p[0] + 0.587f * p[1] + 0.114f * p[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = clamp255(g + (p[k] - g) * sf);
}

// the source rows of a block's RB output rows (LDS windows or global memory,
// each pointing at the box's first byte of the row)
template <int RB>
struct Rows {
  const uint8_t* top[RB];
  const uint8_t* bot[RB];
  float ylerp[RB];
  float xscale;
  int cw, flip;
};

template <int RB>
__device__ __forceinline__ float sample(const Rows<RB>& s, int r, int x, int ch) {
  const Axis xa = axis_weights(x, s.xscale, s.cw);
  const int lo = s.flip ? s.cw - 1 - xa.lo : xa.lo, hi = s.flip ? s.cw - 1 - xa.hi : xa.hi;
  const int a = lo * 3 + ch, b = hi * 3 + ch;
  return lerp2((float)s.top[r][a], (float)s.top[r][b], (float)s.bot[r][a], (float)s.bot[r][b], xa.lerp, s.ylerp[r]);
}

// One output row. MODE 0: no colour step (the arithmetic of
// resize_normalize_kernel), 1: contrast / brightness (per value), 2: with
// saturation, which needs a pixel's three values: a run of 4 values touches
// two pixels, both are computed whole and the run picks its 4 of the 6.
template <typename T, int RB, int MODE>
__device__ __forceinline__ void emit_row(const Rows<RB>& s, int r, const Colour& c, int out_w, float div, float sub,
                                         T* __restrict__ orow) {
#pragma clang fp contract(off)
  const int rv = out_w * 3;
  auto value = [&](int v) {
    const int x = v / 3, ch = v - 3 * x;
    float f = sample(s, r, x, ch);
    if (MODE == 1) f = tone(f, c);
    return f / div - sub;
  };
  auto pixel = [&](int x, float* p) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = tone(sample(s, r, x, k), c);
    saturate(p, c.sf);
  };
  if ((rv & 3) == 0) {  // every row starts 4-value aligned
    typedef __attribute__((ext_vector_type(4))) T T4;
    for (int q = threadIdx.x; q < (rv >> 2); q += IMG_THREADS) {
      T4 o;
      if (MODE == 2) {
        const int x = (4 * q) / 3, k0 = 4 * q - 3 * x;  // the run is values k0 .. k0 + 3 of pixels x, x + 1
        float p[6];
        pixel(x, p);
        pixel(min(x + 1, out_w - 1), p + 3);  // (4q + 3 < rv puts x + 1 inside the row; the min is a guard)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float f = k0 == 0 ? p[j] : k0 == 1 ? p[j + 1] : p[j + 2];
          o[j] = from_f32<T>(f / div - sub);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = from_f32<T>(value(4 * q + j));
      }
      *(T4*)(orow + 4 * q) = o;
    }
  } else if (MODE == 2) {
    for (int x = threadIdx.x; x < out_w; x += IMG_THREADS) {
      float p[3];
      pixel(x, p);
#pragma unroll
      for (int k = 0; k < 3; ++k) orow[3 * x + k] = from_f32<T>(p[k] / div - sub);
    }
  } else {
    for (int v = threadIdx.x; v < rv; v += IMG_THREADS) orow[v] = from_f32<T>(value(v));
  }
}

// resize_normalize_kernel's shape: one block per (image, RB output rows), the
// 2*RB source rows staged in LDS — only the BOX's bytes of each row, so the
// window is sized by the widest box (max_cw), not by the image: a box row
// starts at any byte (x0*3 on top of the packed row start) and stage_row
// handles that and the buffer's last partial piece as for whole rows. The
// flip, the three skip flags and the contrast pivot are block-uniform: one
// branch per block selects the row writer.
template <typename T, int RB, bool USE_LDS>
__global__ __launch_bounds__(IMG_THREADS) void augment_resize_normalize_kernel(
    const fpnmt_image_item* __restrict__ items, const fpnmt_image_aug* __restrict__ aug,
    const unsigned long long* __restrict__ sums, const uint8_t* __restrict__ px, long long px_bytes, int row_words,
    int out_h, int out_w, float div, float sub, T* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ uint32_t lds[];
  const int oy = blockIdx.x * RB, img = blockIdx.y;
  const fpnmt_image_item it = items[img];
  const fpnmt_image_aug a = aug[img];
  const Box bx = clamp_box(it, a);
  const int rv = out_w * 3;  // values per output row
  if (it.h <= 0 || it.w <= 0 || bx.ch <= 0 || bx.cw <= 0) {  // no pixels: keep the output defined
    for (int r = 0; r < RB && oy + r < out_h; ++r) {
      T* orow = out + ((long long)img * out_h + oy + r) * rv;
      for (int x = threadIdx.x; x < rv; x += IMG_THREADS) orow[x] = from_f32<T>(0.f);
    }
    return;
  }
  const int rb = it.w * 3, bb = bx.cw * 3;
  const float yscale = (float)bx.ch / (float)out_h;
  const long long origin = it.offset + (long long)bx.y0 * rb + (long long)bx.x0 * 3;
  Rows<RB> s;
  s.xscale = (float)bx.cw / (float)out_w;
  s.cw = bx.cw;
  s.flip = a.flip != 0;
  // (a box wider than the caller declared reads global memory instead of overrunning LDS)
  const bool staged = USE_LDS && row_window_words(bb) <= row_words;
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    const Axis ya = axis_weights(min(oy + r, out_h - 1), yscale, bx.ch);
    s.ylerp[r] = ya.lerp;
    const long long t0 = origin + (long long)ya.lo * rb, t1 = origin + (long long)ya.hi * rb;
    if (staged) {
      uint32_t* l0 = lds + (2 * r) * row_words;
      uint32_t* l1 = lds + (2 * r + 1) * row_words;
      s.top[r] = (const uint8_t*)l0 + stage_row(l0, px, px_bytes, t0, bb);
      s.bot[r] = (const uint8_t*)l1 + stage_row(l1, px, px_bytes, t1, bb);
    } else {
      s.top[r] = px + t0;
      s.bot[r] = px + t1;
    }
  }
  if (staged) __syncthreads();
  Colour c;
  c.contrast = sums != nullptr && a.contrast != 1.f;
  c.bright = a.brightness != 1.f;
  c.sat = a.saturation != 1.f;
  c.cf = a.contrast, c.bf = a.brightness, c.sf = a.saturation;
  c.m = 0.f;
  if (c.contrast) {  // mean luma of the source box: exact integers, one fp64 divide, one rounding
    const unsigned long long g = 299ull * sums[4LL * img] + 587ull * sums[4LL * img + 1] + 114ull * sums[4LL * img + 2];
    c.m = (float)((double)g / (double)(1000LL * bx.ch * bx.cw));
  }
  const int mode = c.sat ? 2 : (c.contrast || c.bright) ? 1 : 0;
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    if (oy + r >= out_h) break;
    T* orow = out + ((long long)img * out_h + oy + r) * rv;
    if (mode == 0)
      emit_row<T, RB, 0>(s, r, c, out_w, div, sub, orow);
    else if (mode == 1)
      emit_row<T, RB, 1>(s, r, c, out_w, div, sub, orow);
    else
      emit_row<T, RB, 2>(s, r, c, out_w, div, sub, orow);
  }
}

template <typename T>
void augment_launch(const fpnmt_image_item* items, const fpnmt_image_aug* aug, const unsigned long long* sums, int n,
                    const uint8_t* px, long long px_bytes, int max_cw, int out_h, int out_w, float div, float sub,
                    void* out, hipStream_t s) {
  constexpr int RB = 4;
  const int row_words = row_window_words(max_cw * 3);
  const size_t lds4 = 2ull * RB * row_words * 4, lds1 = 2ull * row_words * 4;
  const bool aligned = ((uintptr_t)px & 15) == 0;  // the staging reads 16-B pieces of the packed buffer
  if (aligned && lds4 <= (size_t)IMG_LDS_MAX)
    augment_resize_normalize_kernel<T, RB, true><<<dim3(cdiv(out_h, RB), n), IMG_THREADS, lds4, s>>>(
        items, aug, sums, px, px_bytes, row_words, out_h, out_w, div, sub, (T*)out);
  else if (aligned && lds1 <= (size_t)IMG_LDS_MAX)
    augment_resize_normalize_kernel<T, 1, true><<<dim3(out_h, n), IMG_THREADS, lds1, s>>>(
        items, aug, sums, px, px_bytes, row_words, out_h, out_w, div, sub, (T*)out);
  else
    augment_resize_normalize_kernel<T, 1, false><<<dim3(out_h, n), IMG_THREADS, 0, s>>>(
        items, aug, sums, px, px_bytes, 0, out_h, out_w, div, sub, (T*)out);
}

}  // namespace
}  // namespace fpnmt

using namespace fpnmt;

extern "C" {

int fpnmt_image_crop_stats(const fpnmt_image_item* items_dev, const fpnmt_image_aug* aug_dev, int n,
                           const uint8_t* pixels, long long pixel_bytes, unsigned long long* sums,
                           fpnmt_stream_t stream) {
  if (n < 0 || pixel_bytes < 0) return fail(FPNMT_E_ARG, "image_crop_stats: bad sizes");
  if (n > 65535) return fail(FPNMT_E_UNSUPPORTED, "image_crop_stats: grid too large");
  if (n == 0) return 0;
  if (!items_dev || !aug_dev || !pixels || !sums) return fail(FPNMT_E_ARG, "image_crop_stats: null pointer");
  // (a kernel node: hipMemsetAsync does not re-zero on a graph replay, common.h)
  if (int e = zero_fill(sums, (size_t)n * 4 * sizeof(unsigned long long), (hipStream_t)stream)) return e;
  const int aligned = ((uintptr_t)pixels & 15) == 0;
  image_crop_stats_kernel<<<dim3(STATS_CHUNKS, n), IMG_THREADS, 0, (hipStream_t)stream>>>(
      items_dev, aug_dev, pixels, pixel_bytes, aligned, sums);
  return check_launch("image_crop_stats");
}

int fpnmt_image_augment_resize_normalize(const fpnmt_image_item* items_dev, const fpnmt_image_aug* aug_dev,
                                         const unsigned long long* sums, int n, const uint8_t* pixels,
                                         long long pixel_bytes, int max_cw, int out_h, int out_w, float div,
                                         float sub, int dtype, void* out, fpnmt_stream_t stream) {
  if (dtype != FPNMT_BF16 && dtype != FPNMT_F32)
    return fail(FPNMT_E_ARG, "image_augment_resize_normalize: bad dtype");
  if (n < 0 || out_h <= 0 || out_w <= 0 || max_cw <= 0 || pixel_bytes < 0)
    return fail(FPNMT_E_ARG, "image_augment_resize_normalize: bad sizes");
  if (out_h > 65535 || n > 65535) return fail(FPNMT_E_UNSUPPORTED, "image_augment_resize_normalize: grid too large");
  if (!(div != 0.f)) return fail(FPNMT_E_ARG, "image_augment_resize_normalize: div must be non-zero");
  if (n == 0) return 0;
  if (!items_dev || !aug_dev || !pixels || !out)
    return fail(FPNMT_E_ARG, "image_augment_resize_normalize: null pointer");
  if (dtype == FPNMT_BF16)
    augment_launch<bf16>(items_dev, aug_dev, sums, n, pixels, pixel_bytes, max_cw, out_h, out_w, div, sub, out,
                         (hipStream_t)stream);
  else
    augment_launch<float>(items_dev, aug_dev, sums, n, pixels, pixel_bytes, max_cw, out_h, out_w, div, sub, out,
                          (hipStream_t)stream);
  return check_launch("image_augment_resize_normalize");
}

int fpnmt_image_resize_normalize(const fpnmt_image_item* items_dev, int n, const uint8_t* pixels,
                                 long long pixel_bytes, int max_w, int out_h, int out_w, float div, float sub,
                                 int dtype, void* out, fpnmt_stream_t stream) {
  if (dtype != FPNMT_BF16 && dtype != FPNMT_F32) return fail(FPNMT_E_ARG, "image_resize_normalize: bad dtype");
  if (n < 0 || out_h <= 0 || out_w <= 0 || max_w <= 0 || pixel_bytes < 0)
    return fail(FPNMT_E_ARG, "image_resize_normalize: bad sizes");
  if (out_h > 65535 || n > 65535) return fail(FPNMT_E_UNSUPPORTED, "image_resize_normalize: grid too large");
  if (!(div != 0.f)) return fail(FPNMT_E_ARG, "image_resize_normalize: div must be non-zero");
  if (n == 0) return 0;
  if (!items_dev || !pixels || !out) return fail(FPNMT_E_ARG, "image_resize_normalize: null pointer");
  if (dtype == FPNMT_BF16)
    resize_launch<bf16>(items_dev, n, pixels, pixel_bytes, max_w, out_h, out_w, div, sub, out, (hipStream_t)stream);
  else
    resize_launch<float>(items_dev, n, pixels, pixel_bytes, max_w, out_h, out_w, div, sub, out, (hipStream_t)stream);
  return check_launch("image_resize_normalize");
}

}  // extern "C"
