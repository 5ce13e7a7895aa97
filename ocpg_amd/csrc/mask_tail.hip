// Inference tail of the mask output: stride-4 logits -> what the drivers write, in one pass with no intermediate tensor.
//
// Reference (inference_davis.py:233-261, inference_ytvos.py has the same core; the model's eval branch, models/ocpg.py:371-372, adds
// the nearest x4): F.interpolate(scale_factor=4) of the MSO output, un-pad crop, F.interpolate(size=origin, bilinear,
// align_corners=False), sigmoid, then either `> threshold` (YTVOS, 0 / 255 PNGs) or the multi-object merge (DAVIS: zero below the
// threshold, prepend a constant background plane, argmax over objects).  As ATen passes that chain moves about
// 8 Hp Wp + 19 H0 W0 bytes per frame and object; here every output pixel is computed from the [hs, ws] source (about 100 KB per
// frame, L2-resident) and written once: 4 bytes (mode 0) or 1 byte (modes 1 / 2) per output pixel.
//
// Per output pixel (y, x) of image n:
//   virtual map  V[yy][xx] = src[yy / up][xx / up] for yy < crop_h, xx < crop_w     (nearest replication by `up`, then the crop)
//   bilinear     ATen's align_corners=False rule in fp32, in ATen's operation order (UpSampleBilinear2d: area_pixel_compute_scale /
//                area_pixel_compute_source_index): scale = (float)crop / out; s = scale * (d + 0.5f) - 0.5f, clamped at 0;
//                i0 = (int)s; i1 = i0 + (i0 < crop - 1); l1 = s - i0; l0 = 1 - l1;
//                v = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d)          (the i1 clamp is against the CROP)
//   sigmoid      p = 1 / (1 + expf(-v))                                              (expf, IEEE division: a few ulp of p)
//   mode 0       out fp32 = p
//   mode 1       out uint8 = p > thr ? on_value : 0
//   mode 2       out uint8 = label: candidates [bg, p_1 .. p_K] with p_k < thr replaced by 0, index of the FIRST maximum (ascending scan,
//                strict >: torch.argmax's tie rule)
//
// Shape: wave64, 256-thread workgroups = 4 rows x 64 lanes; a lane owns 4 consecutive output pixels of one row.  The groups of a row
// are laid out from the row's first ALIGNED destination address (16 bytes for fp32, 4 bytes for uint8) at or before its start, so
// every group that lies wholly inside the row is one float4 / one 32-bit store whatever out_w % 4 is; the (at most two) groups that
// straddle a row end are written element by element.  Rows (in fours) are grid.y, images grid.z.  No LDS, no atomics, no
// synchronisation; offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"

namespace {

constexpr int NT = 256;            // threads per workgroup
constexpr int ROWS = NT / 64;      // output rows per workgroup: one wave each
constexpr int PX = 4;              // output pixels per lane

struct Axis {
  int i0, i1;       // source indices in the virtual map
  float l0, l1;
};

__device__ __forceinline__ Axis source_index(float scale, int d, int crop) {
  float s = scale * ((float)d + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  int i0 = (int)s;
  i0 = i0 < crop - 1 ? i0 : crop - 1;        // never taken for d < out (s < crop - 0.5): keeps every read inside the crop regardless
  Axis a;
  a.i0 = i0;
  a.i1 = i0 + (i0 < crop - 1 ? 1 : 0);
  a.l1 = s - (float)i0;
  a.l0 = 1.f - a.l1;
  return a;
}

template <int UP>
__device__ __forceinline__ int down(int i, int up) {
  return UP == 0 ? i / up : i / UP;
}

__device__ __forceinline__ float sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// MODE as in the header; UP: 1, 4, or 0 = run-time `up`
template <int MODE, int UP>
__global__ __launch_bounds__(NT) void mask_tail(const float* __restrict__ src, int K, int N, int hs, int ws, int up, int crop_h, int crop_w,
                                                int out_h, int out_w, float scale_y, float scale_x, float thr, float bg, int on_value,
                                                void* __restrict__ outv) {
  const int y = blockIdx.y * ROWS + (threadIdx.x >> 6);
  if (y >= out_h) return;
  const int n = blockIdx.z;
  const long long row = ((long long)n * out_h + y) * out_w;          // element offset of the row in out
  constexpr int ESZ = MODE == 0 ? 4 : 1;
  const uintptr_t row_addr = reinterpret_cast<uintptr_t>(outv) + (uintptr_t)row * ESZ;
  // elements between the aligned address at or before the row start and the row start (fp32: out is 4-byte aligned as a float*)
  const int shift = MODE == 0 ? (int)((row_addr >> 2) & 3) : (int)(row_addr & 3);
  const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * PX - shift;
  if (x0 >= out_w) return;

  const Axis ay = source_index(scale_y, y, crop_h);
  const int r0 = down<UP>(ay.i0, up), r1 = down<UP>(ay.i1, up);
  int c0[PX], c1[PX];
  float l0x[PX], l1x[PX];
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    int x = x0 + j;
    x = x < 0 ? 0 : (x < out_w ? x : out_w - 1);                     // pixels outside the row are computed on a clamped x, never stored
    const Axis ax = source_index(scale_x, x, crop_w);
    c0[j] = down<UP>(ax.i0, up);
    c1[j] = down<UP>(ax.i1, up);
    l0x[j] = ax.l0;
    l1x[j] = ax.l1;
  }

  const long long plane = (long long)hs * ws;
  float p[PX];
  unsigned lab[PX];
  if (MODE == 2) {
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      p[j] = bg;
      lab[j] = 0u;
    }
  }
  const int nk = MODE == 2 ? K : 1;
  for (int k = 0; k < nk; ++k) {
    const float* s = src + ((long long)k * N + n) * plane;
    const float* s0 = s + (long long)r0 * ws;
    const float* s1 = s + (long long)r1 * ws;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const float a = s0[c0[j]], b = s0[c1[j]], c = s1[c0[j]], d = s1[c1[j]];
      const float v = ay.l0 * (l0x[j] * a + l1x[j] * b) + ay.l1 * (l0x[j] * c + l1x[j] * d);
      const float pk = sigmoid(v);
      if (MODE == 2) {
        const float cand = pk < thr ? 0.f : pk;
        if (cand > p[j]) {
          p[j] = cand;
          lab[j] = (unsigned)(k + 1);
        }
      } else {
        p[j] = pk;
      }
    }
  }

  const bool whole = x0 >= 0 && x0 + PX <= out_w;
  if (MODE == 0) {
    float* o = reinterpret_cast<float*>(outv) + row;
    if (whole && ((row_addr + (uintptr_t)x0 * 4) & 15) == 0) {
      *reinterpret_cast<float4*>(o + x0) = make_float4(p[0], p[1], p[2], p[3]);
    } else {
#pragma unroll
      for (int j = 0; j < PX; ++j)
        if (x0 + j >= 0 && x0 + j < out_w) o[x0 + j] = p[j];
    }
  } else {
    unsigned char* o = reinterpret_cast<unsigned char*>(outv) + row;
    unsigned b[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) b[j] = MODE == 1 ? (p[j] > thr ? (unsigned)on_value : 0u) : lab[j];
    if (whole && ((row_addr + (uintptr_t)x0) & 3) == 0) {
      *reinterpret_cast<unsigned*>(o + x0) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);      // little endian: pixel x0 is the low byte
    } else {
#pragma unroll
      for (int j = 0; j < PX; ++j)
        if (x0 + j >= 0 && x0 + j < out_w) o[x0 + j] = (unsigned char)b[j];
    }
  }
}

template <int MODE>
void launch(dim3 grid, hipStream_t st, const float* src, int K, int N, int hs, int ws, int up, int crop_h, int crop_w, int out_h, int out_w,
            float thr, float bg, int on_value, void* out) {
  const float sy = (float)crop_h / (float)out_h, sx = (float)crop_w / (float)out_w;
  if (up == 4)
    mask_tail<MODE, 4><<<grid, NT, 0, st>>>(src, K, N, hs, ws, up, crop_h, crop_w, out_h, out_w, sy, sx, thr, bg, on_value, out);
  else if (up == 1)
    mask_tail<MODE, 1><<<grid, NT, 0, st>>>(src, K, N, hs, ws, up, crop_h, crop_w, out_h, out_w, sy, sx, thr, bg, on_value, out);
  else
    mask_tail<MODE, 0><<<grid, NT, 0, st>>>(src, K, N, hs, ws, up, crop_h, crop_w, out_h, out_w, sy, sx, thr, bg, on_value, out);
}

}  // namespace

extern "C" int ocpg_mask_tail_f32(const float* src, int K, int N, int hs, int ws, int up, int crop_h, int crop_w, int out_h, int out_w,
                                  int mode, float thr, float bg, int on_value, void* out, void* stream) {
  if (K <= 0 || N <= 0 || hs <= 0 || ws <= 0 || up <= 0 || crop_h <= 0 || crop_w <= 0 || out_h <= 0 || out_w <= 0) return -1006;
  if (mode < 0 || mode > 2) return -2104;
  if (mode != 2 && K != 1) return -2101;
  if (mode == 2 && K > 255) return -2103;
  if ((long long)crop_h > (long long)hs * up || (long long)crop_w > (long long)ws * up) return -2102;
  if (mode == 1 && (on_value < 0 || on_value > 255)) return -2105;
  const long long gy = ((long long)out_h + ROWS - 1) / ROWS;
  if (gy > 65535 || N > 65535) return -1008;
  if (!src) return -1001;
  if (!out) return -1015;
  // a row's groups start up to 3 elements before the row: size grid.x for the largest shift
  const unsigned gx = (unsigned)(((long long)out_w + 3 + 64 * PX - 1) / (64 * PX));
  const dim3 grid(gx, (unsigned)gy, (unsigned)N);
  hipStream_t st = (hipStream_t)stream;
  if (mode == 0)
    launch<0>(grid, st, src, K, N, hs, ws, up, crop_h, crop_w, out_h, out_w, thr, bg, on_value, out);
  else if (mode == 1)
    launch<1>(grid, st, src, K, N, hs, ws, up, crop_h, crop_w, out_h, out_w, thr, bg, on_value, out);
  else
    launch<2>(grid, st, src, K, N, hs, ws, up, crop_h, crop_w, out_h, out_w, thr, bg, on_value, out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
