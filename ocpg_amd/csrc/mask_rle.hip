// COCO run-length encoding of binary masks on the device: planes (or mask logits) -> run counts -> the compressed ASCII string that
// models/postprocessors.py: rle_counts / rle_encode make on the host (the dict pycocotools' `encode` returns), byte for byte.
//
// The format (the public COCO one, restated):
//   order    pixels in COLUMN-major order, k = x * H + y, N = H * W of them
//   counts   runs alternate 0, 1, 0, ...; the first run is the zeros and has length 0 when pixel 0 is set; the last run ends at N
//   string   count c[i] is emitted as x = c[i] - c[i-2] for i > 2 (from the fourth count on) and as c[i] otherwise; x is cut into 5-bit
//            groups, low first, as 2's complement; a group is the last one when the remaining value is 0 and bit 4 of the group is
//            clear, or -1 and bit 4 is set; every other group carries 0x20; every group is offset by 48.  |x| < 2^31: 1..7 characters.
//
// Three passes, each ONE launch over all masks of the call, sizes by value, plain vector stores, no float atomics, no atomics at all,
// no memset.  No workgroup waits for another: a prefix over earlier chunks is read from what the PREVIOUS launch published.
//
//   1 pack     The linear order of a mask is cut into chunks of CHUNK = 4096 pixels = 64 bitmap words; a 256-thread workgroup owns
//              one chunk, each of its 4 waves 16 consecutive words.  A lane owns pixel k; __ballot of the pixel bit over the wave is
//              bits[m][k / 64].  Transitions are t = w ^ ((w << 1) | prev), prev = the last bit of the preceding word; at a wave's
//              first word prev is the bit of pixel k - 1 evaluated again by this wave (no dependence on any other workgroup, nor on
//              another wave), at k = 0 it is 0: a mask that starts set has a transition at position 0, the zero-length first run.
//              Lanes past N are masked out of the ballot and of t.  Per chunk: the number of transitions and the position of the
//              last one (-1: none).  The chunk-0 workgroup also records N.  A second, tiny launch sums the chunk counts per mask into
//              n_trans, which the caller reads back to size `counts`.
//              Two sources: (a) row-major byte planes, read straight down the columns.  With a chunk of 4096 pixels and H of a few
//              hundred a chunk spans about a dozen columns, so a row segment of its tile is a dozen bytes: staging through LDS
//              cannot make a longer coalesced segment than the direct read touches, the lines come from L2 (planes <= 1 MB) and the
//              pass is 29 us for five 720 x 1280 planes, under a tenth of a call that is bound by its two readbacks.
//              (b) mask logits: the pixel function of ocpg_mask_tail_f32 mode 1 (csrc/mask_tail.hip), restated below, negated with
//              `invert`; nothing at the original resolution is written but the bit words.
//              (x, y) of a pixel: one division per wave, then add-and-wrap per word and lane (H >= 64; one division per lane below).
//   2 runs     A workgroup per chunk sums the published counts of the chunks before its own in its mask and takes the largest
//              published position (the last transition before the chunk), recomputes t of its 64 words from the bit words, scans
//              the 64 population counts and last positions in one wave, and then a lane per pixel writes
//              c[first + i] = pos_i - pos_{i-1} (pos_{-1} = 0).  The mask's last chunk appends N - last and n_runs = transitions + 1.
//   3 string   One 1024-thread workgroup per mask loops over blocks of 1024 runs with a running carry: per run the delta-coded value
//              and its character count, an exclusive scan (wave shuffles, wave totals through LDS, one barrier per block), the
//              characters.  n_bytes[m] goes to device memory.
//
// Everything the kernels read of the workspace and of the outputs they wrote themselves in this call.  Geometry, run starts and run
// numbers read from device memory are clamped before they address anything.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"

namespace {

constexpr int CHUNK = 4096;              // pixels per chunk (a workgroup of pass 1 and of pass 2)
constexpr int WORDS = CHUNK / 64;        // bitmap words per chunk
constexpr int NT = 256;                  // threads per workgroup, passes 1 and 2
constexpr int WPW = WORDS / (NT / 64);   // words per wave
constexpr int NT3 = 1024;                // threads per workgroup, pass 3
static_assert(WORDS == 64, "pass 2 scans a chunk's words in one wave");
static_assert(WPW <= 64, "a lane keeps one of its wave's words");

typedef unsigned long long u64;

struct Workspace {
  u64* bits;       // [n_masks, max_chunks, WORDS]
  int* ctab;       // [n_masks, max_chunks, 2]: transitions in the chunk, position of the last one or -1
  int* npx;        // [n_masks]: N as pass 1 clamped it
};

__host__ __device__ inline long long chunks_of(long long n) { return (n + CHUNK - 1) / CHUNK; }

inline long long workspace_bytes(int n_masks, long long max_n) {
  const long long mc = chunks_of(max_n);
  return (long long)n_masks * mc * WORDS * 8 + (long long)n_masks * mc * 8 + (((long long)n_masks * 4 + 7) & ~7ll);
}

inline Workspace carve(void* p, int n_masks, long long max_n) {
  const long long mc = chunks_of(max_n);
  Workspace w;
  w.bits = (u64*)p;
  w.ctab = (int*)(w.bits + (long long)n_masks * mc * WORDS);
  w.npx = w.ctab + (long long)n_masks * mc * 2;
  return w;
}

// ---- pass 1 --------------------------------------------------------------------------------------------------------------------------
// pix(y, x) -> bool for y < H, x < N / H; called by whole waves on valid pixels only
template <class F>
__device__ __forceinline__ void pack_chunk(int m, int H, int N, int max_chunks, Workspace ws, F pix) {
  __shared__ int s_cnt[NT / 64], s_last[NT / 64];
  const unsigned c = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned n = (unsigned)N;
  unsigned kb = c * CHUNK + wave * (WPW * 64);                   // the wave's first pixel: < 2^31 + CHUNK, fits 32 bits unsigned
  u64 prev = 0;
  if (kb > 0 && kb - 1 < n) {
    const unsigned kk = kb - 1, xx = kk / (unsigned)H;
    prev = pix((int)(kk - xx * H), (int)xx) ? 1ull : 0ull;
  }
  unsigned xb = kb / (unsigned)H, yb = kb - xb * (unsigned)H;   // per wave; carried word to word below when H >= 64
  int cnt = 0, last = -1;
  u64 mine = 0;
#pragma unroll 1
  for (int j = 0; j < WPW; ++j, kb += 64) {
    const unsigned k = kb + lane;
    unsigned x, y;
    if (H >= 64) {
      y = yb + lane;
      x = xb;
      if (y >= (unsigned)H) {
        y -= H;
        ++x;
      }
      yb += 64;
      if (yb >= (unsigned)H) {
        yb -= H;
        ++xb;
      }
    } else {
      x = k / (unsigned)H;
      y = k - x * (unsigned)H;
    }
    bool bit = false;
    if (k < n) bit = pix((int)y, (int)x);
    const u64 w = __ballot(bit);
    const unsigned nvalid = kb >= n ? 0u : (n - kb >= 64u ? 64u : n - kb);
    const u64 vm = nvalid >= 64u ? ~0ull : ((1ull << nvalid) - 1ull);
    const u64 t = (w ^ ((w << 1) | prev)) & vm;
    cnt += __popcll(t);
    if (t) last = (int)(kb + 63u - (unsigned)__clzll((long long)t));
    if (lane == j) mine = w;
    prev = w >> 63;
  }
  const long long chunk = (long long)m * max_chunks + c;
  if (lane < WPW) ws.bits[chunk * WORDS + wave * WPW + lane] = mine;
  if (lane == 0) {
    s_cnt[wave] = cnt;
    s_last[wave] = last;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int a = 0, b = -1;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
      a += s_cnt[i];
      b = s_last[i] > b ? s_last[i] : b;
    }
    ws.ctab[chunk * 2] = a;
    ws.ctab[chunk * 2 + 1] = b;
    if (c == 0) ws.npx[m] = N;
  }
}

// clamp (h, w) read from device memory: 1 <= h, 1 <= w, h * w <= max_n; false when nothing of the mask can be served
__device__ __forceinline__ bool clamp_size(int& h, int& w, long long max_n) {
  if (h <= 0 || w <= 0) return false;
  if (h > max_n) h = (int)max_n;
  const long long wm = max_n / h;
  if (w > wm) w = (int)wm;
  return true;
}

__global__ __launch_bounds__(NT) void rle_pack_planes(const unsigned char* __restrict__ base, const long long* __restrict__ off,
                                                      const int* __restrict__ geom, long long max_n, int max_chunks, Workspace ws) {
  const int m = blockIdx.y;
  int H = geom[2 * m], W = geom[2 * m + 1];
  if (!clamp_size(H, W, max_n)) return;
  const int N = H * W;
  if ((long long)blockIdx.x >= chunks_of(N)) return;
  const unsigned char* p = base + off[m];
  pack_chunk(m, H, N, max_chunks, ws, [=](int y, int x) { return p[(long long)y * W + x] != 0; });
}

// the pixel function of csrc/mask_tail.hip (mode 1), restated: same expressions in the same order
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

// UP: 1, 4, or 0 = run-time `up`
template <int UP>
__global__ __launch_bounds__(NT) void rle_pack_logits(const float* __restrict__ src, int Q, int hs, int ws_, int up,
                                                      const int* __restrict__ geom, long long max_n, int max_chunks, float thr, int invert,
                                                      Workspace ws) {
  const int m = blockIdx.y, b = m / Q;
  int crop_h = geom[4 * b + 0], crop_w = geom[4 * b + 1], H = geom[4 * b + 2], W = geom[4 * b + 3];
  crop_h = crop_h < hs * up ? crop_h : hs * up;
  crop_w = crop_w < ws_ * up ? crop_w : ws_ * up;
  if (crop_h <= 0 || crop_w <= 0 || !clamp_size(H, W, max_n)) return;
  const int N = H * W;
  if ((long long)blockIdx.x >= chunks_of(N)) return;
  const float* s = src + (long long)m * hs * ws_;
  const float scale_y = (float)crop_h / (float)H, scale_x = (float)crop_w / (float)W;
  pack_chunk(m, H, N, max_chunks, ws, [=](int y, int x) {
    const Axis ay = source_index(scale_y, y, crop_h), ax = source_index(scale_x, x, crop_w);
    const float* s0 = s + (long long)down<UP>(ay.i0, up) * ws_;
    const float* s1 = s + (long long)down<UP>(ay.i1, up) * ws_;
    const int c0 = down<UP>(ax.i0, up), c1 = down<UP>(ax.i1, up);
    const float a = s0[c0], bb = s0[c1], c = s1[c0], d = s1[c1];
    const float v = ay.l0 * (ax.l0 * a + ax.l1 * bb) + ay.l1 * (ax.l0 * c + ax.l1 * d);
    const bool on = sigmoid(v) > thr;
    return invert ? !on : on;
  });
}

// n_trans[m] = the sum of the mask's chunk counts: one wave per mask
__global__ __launch_bounds__(64) void rle_totals(int n_masks, int max_chunks, Workspace ws, int* __restrict__ n_trans) {
  const int m = blockIdx.x;
  int N = ws.npx[m];
  N = N < 0 ? 0 : N;
  long long nch = chunks_of(N);
  nch = nch < max_chunks ? nch : max_chunks;
  int a = 0;
  for (long long j = threadIdx.x; j < nch; j += 64) a += ws.ctab[((long long)m * max_chunks + j) * 2];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) a += __shfl_xor(a, d);
  if (threadIdx.x == 0) n_trans[m] = a;
}

// ---- pass 2 --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void rle_runs(long long max_n, int max_chunks, Workspace ws, const long long* __restrict__ run_start,
                                               long long cap, int* __restrict__ counts, int* __restrict__ n_runs) {
  __shared__ int s_sum[NT / 64], s_max[NT / 64];
  __shared__ u64 s_t[WORDS];
  __shared__ int s_base[WORDS], s_prev[WORDS];
  const int m = blockIdx.y;
  const unsigned c = blockIdx.x;
  long long N = ws.npx[m];
  N = N < 0 ? 0 : (N > max_n ? max_n : N);
  const long long nch = chunks_of(N);
  if ((long long)c >= nch) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = (long long)m * max_chunks;
  // the chunks before this one: their transitions and the last position among them
  int a = 0, b = -1;
  for (unsigned j = threadIdx.x; j < c; j += NT) {
    a += ws.ctab[(row + j) * 2];
    const int l = ws.ctab[(row + j) * 2 + 1];
    b = l > b ? l : b;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    a += __shfl_xor(a, d);
    const int o = __shfl_xor(b, d);
    b = o > b ? o : b;
  }
  if (lane == 0) {
    s_sum[wave] = a;
    s_max[wave] = b;
  }
  // this chunk's transition words, their exclusive count prefix and the last transition before each word: wave 0, a lane per word
  const unsigned n = (unsigned)N, k0 = c * CHUNK;
  if (wave == 0) {
    const u64 w = ws.bits[(row + c) * WORDS + lane];
    const u64 wb = __shfl_up(w, 1);                    // executed by every lane
    u64 prev = 0;
    if (lane > 0) prev = wb >> 63;
    else if (c > 0) prev = ws.bits[(row + c) * WORDS - 1] >> 63;
    const unsigned kw = k0 + 64u * lane;
    const unsigned nvalid = kw >= n ? 0u : (n - kw >= 64u ? 64u : n - kw);
    const u64 vm = nvalid >= 64u ? ~0ull : ((1ull << nvalid) - 1ull);
    const u64 t = (w ^ ((w << 1) | prev)) & vm;
    int inc = __popcll(t);
    int lastp = t ? (int)(kw + 63u - (unsigned)__clzll((long long)t)) : -1;
    const int own = inc;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int oi = __shfl_up(inc, d), ol = __shfl_up(lastp, d);
      if (lane >= d) {
        inc += oi;
        lastp = ol > lastp ? ol : lastp;
      }
    }
    const int before = __shfl_up(lastp, 1);            // inclusive maximum of the words before this one
    s_t[lane] = t;
    s_base[lane] = inc - own;
    s_prev[lane] = lane > 0 ? before : -1;
  }
  __syncthreads();
  int first = 0, lastb = -1;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) {
    first += s_sum[i];
    lastb = s_max[i] > lastb ? s_max[i] : lastb;
  }
  long long start = run_start[m];
  start = start < 0 ? 0 : (start > cap ? cap : start);
  int* out = counts + start;
  const long long room = cap - start;                  // runs this mask may write
#pragma unroll 1
  for (int j = 0; j < WPW; ++j) {
    const int wi = wave * WPW + j;
    const u64 t = s_t[wi];
    if (t == 0) continue;                              // uniform over the wave
    const u64 below = t & ((1ull << lane) - 1ull);
    if ((t >> lane) & 1ull) {
      const int pos = (int)(k0 + 64u * wi) + lane;
      int prevpos = below ? (int)(k0 + 64u * wi) + 63 - __clzll((long long)below) : s_prev[wi];
      prevpos = prevpos < 0 ? lastb : prevpos;
      prevpos = prevpos < 0 ? 0 : prevpos;
      const long long idx = (long long)first + s_base[wi] + __popcll(below);
      if (idx < room) out[idx] = pos - prevpos;
    }
  }
  if ((long long)c == nch - 1 && threadIdx.x == 0) {
    const int total = first + s_base[WORDS - 1] + __popcll(s_t[WORDS - 1]);
    int lastall = s_prev[WORDS - 1];
    if (s_t[WORDS - 1]) lastall = (int)(k0 + 64u * (WORDS - 1)) + 63 - __clzll((long long)s_t[WORDS - 1]);
    lastall = lastall < 0 ? lastb : lastall;
    lastall = lastall < 0 ? 0 : lastall;
    if (total < room) out[total] = (int)N - lastall;
    n_runs[m] = total + 1;
  }
}

// ---- pass 3 --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT3) void rle_string(const long long* __restrict__ run_start, long long cap, const int* __restrict__ counts,
                                                  const int* __restrict__ n_runs, unsigned char* __restrict__ bytes,
                                                  long long* __restrict__ n_bytes) {
  __shared__ int s_tot[2][NT3 / 64];
  const int m = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long start = run_start[m];
  start = start < 0 ? 0 : (start > cap ? cap : start);
  long long nr = n_runs[m];
  nr = nr < 0 ? 0 : (nr > cap - start ? cap - start : nr);
  const int* c = counts + start;
  unsigned char* o = bytes + 7 * start;                // at most 7 characters per run: the string of mask m has room for all its runs
  long long carry = 0;
  int buf = 0;
  for (long long i0 = 0; i0 < nr; i0 += NT3, buf ^= 1) {
    const long long i = i0 + threadIdx.x;
    int x = 0, nch = 0;
    if (i < nr) {
      x = c[i];
      if (i > 2) x -= c[i - 2];
      int v = x;
      bool more = true;
      while (more) {                                   // 32-bit arithmetic shift: the host loop on a value of |x| < 2^31
        const int ch = v & 0x1f;
        v >>= 5;
        more = (ch & 0x10) ? v != -1 : v != 0;
        ++nch;
      }
    }
    int inc = nch;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int oi = __shfl_up(inc, d);
      if (lane >= d) inc += oi;
    }
    if (lane == 63) s_tot[buf][wave] = inc;
    __syncthreads();                                   // one barrier per block: the totals alternate between two rows
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NT3 / 64; ++w) {
      const int t = s_tot[buf][w];
      before += w < wave ? t : 0;
      all += t;
    }
    if (i < nr) {
      unsigned char* p = o + carry + before + (inc - nch);
      int v = x;
      for (int k = 0; k < nch; ++k) {
        int ch = v & 0x1f;
        v >>= 5;
        if (k + 1 < nch) ch |= 0x20;
        p[k] = (unsigned char)(ch + 48);
      }
    }
    carry += all;
  }
  if (threadIdx.x == 0) n_bytes[m] = carry;
}

}  // namespace

// host-side query, nothing is launched (the stream is taken like every entry of the family and not used)
extern "C" int ocpg_mask_rle_query(int n_masks, long long max_n, long long* workspace_bytes_host, int* chunk_pixels_host, void* stream) {
  (void)stream;
  if (n_masks <= 0 || max_n <= 0) return -1006;
  if (max_n >= (1ll << 31)) return -2603;
  if (n_masks > 65535) return -1008;
  if (workspace_bytes_host) *workspace_bytes_host = workspace_bytes(n_masks, max_n);
  if (chunk_pixels_host) *chunk_pixels_host = CHUNK;
  return 0;
}

namespace {

// the checks the two pack entries share, in the documented order; mc = chunks of the largest mask
int pack_common(int n_masks, long long max_n, const int* n_trans, const void* workspace) {
  if (max_n >= (1ll << 31)) return -2603;
  if (n_masks > 65535) return -1008;
  if (!n_trans) return -1015;
  if (!workspace || ((uintptr_t)workspace & 7)) return -2606;
  return 0;
}

}  // namespace

extern "C" int ocpg_mask_rle_pack_u8(const unsigned char* base, const long long* off, int n_masks, const int* geom_host, const int* geom,
                                     long long max_n, int* n_trans, void* workspace, void* stream) {
  if (n_masks <= 0 || max_n <= 0) return -1006;
  if (!geom_host || !geom) return -2605;
  for (int m = 0; m < n_masks; ++m) {
    const int* g = geom_host + 2 * (long long)m;
    if (g[0] <= 0 || g[1] <= 0) return -1006;
    if ((long long)g[0] * g[1] >= (1ll << 31)) return -2603;
    if ((long long)g[0] * g[1] > max_n) return -2604;
  }
  const int rc = pack_common(n_masks, max_n, n_trans, workspace);
  if (rc) return rc;
  if (!base || !off) return -1001;
  const Workspace ws = carve(workspace, n_masks, max_n);
  const int mc = (int)chunks_of(max_n);
  hipStream_t st = (hipStream_t)stream;
  rle_pack_planes<<<dim3((unsigned)mc, (unsigned)n_masks), NT, 0, st>>>(base, off, geom, max_n, mc, ws);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return -(int)e;
  rle_totals<<<n_masks, 64, 0, st>>>(n_masks, mc, ws, n_trans);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

extern "C" int ocpg_mask_rle_pack_logits_f32(const float* src, int B, int Q, int hs, int ws_, int up, const int* geom_host, const int* geom,
                                             long long max_n, float thr, int invert, int* n_trans, void* workspace, void* stream) {
  if (B <= 0 || Q <= 0 || hs <= 0 || ws_ <= 0 || up <= 0 || max_n <= 0) return -1006;
  if (invert != 0 && invert != 1) return -2601;
  if (!geom_host || !geom) return -2605;
  const long long vh = (long long)hs * up, vw = (long long)ws_ * up;
  for (int b = 0; b < B; ++b) {
    const int* g = geom_host + 4 * (long long)b;
    if (g[0] <= 0 || g[1] <= 0 || g[2] <= 0 || g[3] <= 0) return -1006;
    if (g[0] > vh || g[1] > vw) return -2602;
    if ((long long)g[2] * g[3] >= (1ll << 31)) return -2603;
    if ((long long)g[2] * g[3] > max_n) return -2604;
  }
  if ((long long)B * Q > 65535 || vh > 2147483647ll || vw > 2147483647ll) return -1008;
  const int n_masks = B * Q;
  const int rc = pack_common(n_masks, max_n, n_trans, workspace);
  if (rc) return rc;
  if (!src) return -1001;
  const Workspace ws = carve(workspace, n_masks, max_n);
  const int mc = (int)chunks_of(max_n);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)mc, (unsigned)n_masks);
  if (up == 4)
    rle_pack_logits<4><<<grid, NT, 0, st>>>(src, Q, hs, ws_, up, geom, max_n, mc, thr, invert, ws);
  else if (up == 1)
    rle_pack_logits<1><<<grid, NT, 0, st>>>(src, Q, hs, ws_, up, geom, max_n, mc, thr, invert, ws);
  else
    rle_pack_logits<0><<<grid, NT, 0, st>>>(src, Q, hs, ws_, up, geom, max_n, mc, thr, invert, ws);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return -(int)e;
  rle_totals<<<n_masks, 64, 0, st>>>(n_masks, mc, ws, n_trans);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

extern "C" int ocpg_mask_rle_encode(int n_masks, long long max_n, const int* n_trans_host, const long long* run_start_host,
                                    const long long* run_start, long long counts_cap, int* counts, int* n_runs, unsigned char* bytes,
                                    long long* n_bytes, void* workspace, void* stream) {
  if (n_masks <= 0 || max_n <= 0 || counts_cap <= 0) return -1006;
  if (max_n >= (1ll << 31)) return -2603;
  if (n_masks > 65535) return -1008;
  if (!n_trans_host || !run_start_host || !run_start) return -2605;
  long long at = 0;
  for (int m = 0; m < n_masks; ++m) {
    // each mask's runs behind the previous mask's, inside the capacity: transitions + 1 of them
    if (n_trans_host[m] < 0 || run_start_host[m] < at) return -2607;
    at = run_start_host[m] + (long long)n_trans_host[m] + 1;
    if (at > counts_cap) return -2607;
  }
  if (!workspace || ((uintptr_t)workspace & 7)) return -2606;
  if (!counts || !n_runs || !bytes || !n_bytes) return -1015;
  const Workspace ws = carve(workspace, n_masks, max_n);
  const int mc = (int)chunks_of(max_n);
  hipStream_t st = (hipStream_t)stream;
  rle_runs<<<dim3((unsigned)mc, (unsigned)n_masks), NT, 0, st>>>(max_n, mc, ws, run_start, counts_cap, counts, n_runs);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return -(int)e;
  rle_string<<<n_masks, NT3, 0, st>>>(run_start, counts_cap, counts, n_runs, bytes, n_bytes);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
