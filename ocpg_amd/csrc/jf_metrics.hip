// DAVIS-2017 J&F scoring reduced to integer counts: per (pair, frame) the six numbers from which region similarity J and boundary
// accuracy F follow (reference davis2017/metrics.py: db_eval_iou, f_measure, _seg2bmap; the fp64 arithmetic on the counts is
// ocpg_amd/metrics.py:jf_from_counts).
//
// Per pair (result id, ground-truth id) and frame, on label maps gt / res [T, H, W] uint8:
//   A = (res == id_r) & ~void,  B = (gt == id_g) & ~void,  void = (gt == void_label)
//   b(M)  the reference's _seg2bmap at equal size: for y < H-1, x < W-1  (M^M[y,x+1]) | (M^M[y+1,x]) | (M^M[y+1,x+1]); last row
//         M^M[y,x+1]; last column M^M[y+1,x]; corner 0
//   a boundary pixel of one map is matched if the other map has a boundary pixel at an in-image offset dx^2 + dy^2 <= radius^2
//         (cv2.dilate with skimage's disk(radius); pixels outside the image never win)
//   counts = |A&B|, |A|B|, |b(A)|, |b(B)|, matched b(A), matched b(B)
//
// Shape: one 256-thread workgroup per (64 x 32 tile, frame, pair).  A tile starts at a multiple of 64 columns, so with radius <= 64
// everything its pixels can see lies in the three 64-column words around it: both maps are bit-packed in LDS, one bit per pixel,
// rows of 64-bit words.
//   1. masks      a wave per (row, word): 64 lanes load 64 label bytes of each map, __ballot packs A and B.  Rows y0-r .. y0+32+r,
//                 4 words from column x0-64 (the fourth only for its first bit, and only when r = 64); pixels outside the image or
//                 outside the columns the tile needs are not loaded and read as 0.
//   2. boundaries a thread per (row, word): word-wide XORs of the mask with its right / lower / lower-right neighbours.  The
//                 last-row / last-column rules and the zeroing of everything outside the image are column masks and row tests
//                 against the IMAGE (H, W), never the tile.
//   3. counts     popcounts of the tile's own word.  Where the tile has boundary pixels of one map, the other map's boundary is
//                 dilated: per (tile row, dy) the source row is spread horizontally by hw(dy) = floor(sqrt(r^2 - dy^2)) in
//                 O(log hw) shift-ORs of the 192-bit row, the rows are ORed per tile row (LDS atomics), and matched =
//                 popcount(boundary & dilated).  Rows without boundary pixels on either side are skipped.
// The six per-tile counts are summed in LDS and added to counts[pair][frame] with one integer atomic each (only non-zero ones);
// counts is zeroed by a fill kernel first (never hipMemsetAsync: fill.h).  Integer arithmetic throughout: the result does not depend
// on the order of the adds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"
#include "fill.h"

namespace {

typedef unsigned long long u64;

constexpr int NT = 256;          // threads per workgroup
constexpr int TW = 64;           // tile width: one word
constexpr int TH = 32;           // tile height
constexpr int RMAX = 64;         // largest served radius: the halo is one word each side
constexpr int MW = 4;            // mask words per row (columns x0-64 .. x0+191)
constexpr int BW = 3;            // boundary words per row (columns x0-64 .. x0+127)
constexpr int MROWS = TH + 2 * RMAX + 1;
constexpr int BROWS = TH + 2 * RMAX;

// bits j of a word whose bit 0 is column cb with cb + j < n
__device__ __forceinline__ u64 cols_below(int cb, int n) {
  const int c = n - cb;
  return c <= 0 ? 0ull : (c >= 64 ? ~0ull : ((1ull << c) - 1ull));
}

// bits [s, s + 64) of the 128-bit value hi:lo, 0 <= s <= 64
__device__ __forceinline__ u64 shr2(u64 lo, u64 hi, int s) {
  return s == 0 ? lo : (s == 64 ? hi : ((lo >> s) | (hi << (64 - s))));
}

// middle word of the 192-bit row w0:w1:w2 (bit = column, ascending) dilated horizontally by h, 0 <= h <= 64
__device__ __forceinline__ u64 hdilate_mid(u64 w0, u64 w1, u64 w2, int h) {
  // d_k[p] = OR of src[p .. p+k-1]; d_2k = d_k | d_k >> k; last step by n - k <= k
  const int n = 2 * h + 1;
  int k = 1;
  while (2 * k <= n) {
    w0 |= shr2(w0, w1, k);
    w1 |= shr2(w1, w2, k);
    w2 |= shr2(w2, 0ull, k);
    k *= 2;
  }
  if (k < n) {
    const int s = n - k;
    w0 |= shr2(w0, w1, s);
    w1 |= shr2(w1, w2, s);
  }
  // out[x] = d_n[x - h] for the columns of the middle word
  return shr2(w0, w1, 64 - h);
}

__global__ __launch_bounds__(NT) void jf_counts(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ res, int H, int W,
                                                int G, int radius, int void_label, int all_pairs, int tiles_x, int T,
                                                int* __restrict__ counts) {
  __shared__ u64 mA[MROWS][MW], mB[MROWS][MW];
  __shared__ u64 bA[BROWS][BW], bB[BROWS][BW];
  __shared__ u64 dil[2][TH];          // [0] dilated b(B), [1] dilated b(A), the tile's own word
  __shared__ int hw[RMAX + 1];
  __shared__ int cnt[6];

  const int tid = threadIdx.x;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int t = blockIdx.y, p = blockIdx.z;
  const int id_r = (all_pairs ? p / G : p) + 1, id_g = (all_pairs ? p % G : p) + 1;
  const int x0 = tx * TW, y0 = ty * TH;
  const int r = radius;
  const int brows = TH + 2 * r, mrows = brows + 1;

  if (tid < 6) cnt[tid] = 0;
  if (tid < TH) dil[0][tid] = dil[1][tid] = 0ull;
  if (tid <= r) {                                                     // half-widths of the disk's rows, exact integer square root
    const int v = r * r - tid * tid;
    int h = (int)sqrtf((float)v);
    while ((h + 1) * (h + 1) <= v) ++h;
    while (h * h > v) --h;
    hw[tid] = h;
  }

  // 1. masks
  {
    const int lane = tid & 63, wave = tid >> 6;
    const unsigned char* g0 = gt + (long long)t * H * W;
    const unsigned char* s0 = res + (long long)t * H * W;
    const int xlo = x0 - r, xhi = x0 + TW + r;                       // columns the tile needs, inclusive (xhi: right neighbour of the last)
    for (int i = wave; i < mrows * MW; i += NT / 64) {
      const int row = i / MW, w = i % MW;
      const int y = y0 - r + row, x = x0 - 64 + 64 * w + lane;
      bool a = false, b = false;
      if (y >= 0 && y < H && x >= 0 && x < W && x >= xlo && x <= xhi) {
        const long long o = (long long)y * W + x;
        const int gv = g0[o], sv = s0[o];
        const bool keep = gv != void_label;                          // void_label -1 never equals a byte
        a = sv == id_r && keep;
        b = gv == id_g && keep;
      }
      const u64 wa = __ballot(a), wb = __ballot(b);
      if (lane == 0) {
        mA[row][w] = wa;
        mB[row][w] = wb;
      }
    }
  }
  __syncthreads();

  // 2. boundaries: rows y0-r .. y0+TH-1+r, words 0..2
  for (int i = tid; i < brows * BW; i += NT) {
    const int row = i / BW, w = i % BW;
    const int y = y0 - r + row, cb = x0 - 64 + 64 * w;
    u64 va = 0ull, vb = 0ull;
    if (y >= 0 && y < H) {
      const u64 ge0 = ~cols_below(cb, 0);
      const u64 lt = cols_below(cb, W - 1) & ge0;                    // x < W-1: has a right neighbour in the image
      const u64 le = cols_below(cb, W) & ge0;                        // x <= W-1
      {
        const u64 m = mA[row][w], e = (m >> 1) | (mA[row][w + 1] << 63);
        if (y < H - 1) {
          const u64 d = mA[row + 1][w], de = (d >> 1) | (mA[row + 1][w + 1] << 63);
          va = (((m ^ e) | (m ^ de)) & lt) | ((m ^ d) & le);
        } else {
          va = (m ^ e) & lt;
        }
      }
      {
        const u64 m = mB[row][w], e = (m >> 1) | (mB[row][w + 1] << 63);
        if (y < H - 1) {
          const u64 d = mB[row + 1][w], de = (d >> 1) | (mB[row + 1][w + 1] << 63);
          vb = (((m ^ e) | (m ^ de)) & lt) | ((m ^ d) & le);
        } else {
          vb = (m ^ e) & lt;
        }
      }
    }
    bA[row][w] = va;
    bB[row][w] = vb;
  }
  __syncthreads();

  // 3. counts of the tile's own word (row r + yi, word 1)
  if (tid < TH) {
    const u64 a = mA[r + tid][1], b = mB[r + tid][1];
    const int c0 = __popcll(a & b), c1 = __popcll(a | b), c2 = __popcll(bA[r + tid][1]), c3 = __popcll(bB[r + tid][1]);
    if (c0) atomicAdd(&cnt[0], c0);
    if (c1) atomicAdd(&cnt[1], c1);
    if (c2) atomicAdd(&cnt[2], c2);
    if (c3) atomicAdd(&cnt[3], c3);
  }
  __syncthreads();
  const bool needB = cnt[2] > 0, needA = cnt[3] > 0;                   // uniform over the workgroup
  if (needA || needB) {
    const int yi = tid % TH;
    const u64 ownA = bA[r + yi][1], ownB = bB[r + yi][1];
    u64 dB = 0ull, dA = 0ull;
    for (int dyi = tid / TH; dyi <= 2 * r; dyi += NT / TH) {
      const int src = yi + dyi;                                        // boundary row of image row y0 + yi + (dyi - r)
      const int h = hw[dyi < r ? r - dyi : dyi - r];
      if (needB && ownA) {
        const u64 w0 = bB[src][0], w1 = bB[src][1], w2 = bB[src][2];
        if (w0 | w1 | w2) dB |= hdilate_mid(w0, w1, w2, h);
      }
      if (needA && ownB) {
        const u64 w0 = bA[src][0], w1 = bA[src][1], w2 = bA[src][2];
        if (w0 | w1 | w2) dA |= hdilate_mid(w0, w1, w2, h);
      }
    }
    if (dB) atomicOr(&dil[0][yi], dB);
    if (dA) atomicOr(&dil[1][yi], dA);
    __syncthreads();
    if (tid < TH) {
      const int c4 = __popcll(ownA & dil[0][tid]), c5 = __popcll(ownB & dil[1][tid]);
      if (c4) atomicAdd(&cnt[4], c4);
      if (c5) atomicAdd(&cnt[5], c5);
    }
    __syncthreads();
  }
  if (tid < 6) {
    const int c = cnt[tid];
    if (c) atomicAdd(&counts[((long long)p * T + t) * 6 + tid], c);
  }
}

}  // namespace

extern "C" int ocpg_jf_counts_u8(const unsigned char* gt, const unsigned char* res, int T, int H, int W, int G, int R, int radius,
                                 int void_label, int all_pairs, int* counts, void* stream) {
  if (T <= 0 || H <= 0 || W <= 0 || G <= 0 || (all_pairs && R <= 0)) return -1006;
  if (all_pairs != 0 && all_pairs != 1) return -2201;
  if (radius < 1 || radius > RMAX) return -2202;
  if (G > 254 || (all_pairs && R > 254)) return -2203;
  if (void_label < -1 || void_label > 255) return -2204;
  if ((long long)H * W >= (1ll << 31)) return -2205;
  const long long P = all_pairs ? (long long)R * G : G;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const long long tiles = (long long)tiles_x * tiles_y;
  if (tiles > 2147483647ll || T > 65535 || P > 65535) return -1008;
  if (!gt || !res) return -1001;
  if (!counts) return -1015;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = ocpg_fill::zero_async(counts, (size_t)(P * T * 6) * sizeof(int), st);
  if (e != hipSuccess) return -(int)e;
  jf_counts<<<dim3((unsigned)tiles, (unsigned)T, (unsigned)P), NT, 0, st>>>(gt, res, H, W, G, radius, void_label, all_pairs, tiles_x, T,
                                                                           counts);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
