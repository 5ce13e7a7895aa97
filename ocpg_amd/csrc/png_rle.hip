// Run-length deflate of 8-bit planes on the device: the zlib body of a PNG's IDAT chunk for a mask or a label map, byte for byte what
// models/ops/functions/png_func.py composes on the host.
//
// The stream (restated; filter type 0 on every row, so the "filtered data" of an H x W plane is H rows of 0x00 + the row's W bytes):
//   row      a fixed-Huffman block header (BFINAL = 0, BTYPE = 01: the bits 0, 1, 0), the row's tokens, end-of-block (symbol 256, seven
//            zero bits), an empty stored block (the bits 0, 0, 0, zero padding to the byte boundary, 00 00 FF FF).  Every row ends
//            byte-aligned and is coded on its own: rows are made in parallel and concatenated by byte offset.
//   tokens   the W + 1 filtered bytes of the row are cut into maximal runs of equal bytes; a run of value v and length n is the
//            literal v, then with r = n - 1: r / 258 matches of length 258 at distance 1, then one match of length r % 258 at
//            distance 1 when that is >= 3, that many more literals v otherwise.
//   end      after the last row a final block: BFINAL = 1, BTYPE = 01, symbol 256: the two bytes 03 00.
//   codes    RFC 1951 section 3.2.6: literals 0..143 are 0x30 + s in 8 bits, 144..255 are 0x190 + (s - 144) in 9 bits, symbols 256..279
//            are s - 256 in 7 bits, 280..287 are 0xC0 + (s - 280) in 8 bits; length l = len - 3 below 8 is symbol 257 + l without
//            extra bits, 258 is symbol 285 without extra bits, every other length has e = msb(l) - 2 extra bits l & (2^e - 1) and
//            symbol 257 + 4 e + (l >> e); distance 1 is five zero bits.  Bytes fill from the least-significant bit; Huffman codes
//            enter most-significant bit first (stored bit-reversed), extra bits least-significant first.
//
// Count, scan, emit: three launches for any number of planes, no workgroup waits for another, no global atomics, no memset.
//   1 count   one WAVE per row.  The row is walked in groups of 64 filtered bytes, a lane per byte: a lane is the END of a run when its
//             successor differs (the successor of a group's last lane is the first byte of the next group, which the wave has already
//             loaded; past the row it is -1); the ballot of the ends gives every end its predecessor (the highest end below the lane,
//             or the last end of the earlier groups, a wave-uniform carry), hence its run length and the bits of its tokens.  The row's
//             byte length, sum(d) and sum(p * d) over its filtered positions p go to the workspace.
//   2 scan    one workgroup per plane sums the row lengths of the planes before its own, scans its own rows into byte offsets from the
//             start of the output, and reduces the plane's totals: bytes, S0 = sum(d_i), S1 = sum(i * d_i) over the plane's
//             filtered data, in 64 bits (S1 <= 255 n^2 / 2 < 2^63 for n <= 65535 * 4097).  The caller reads them back to size the
//             output and to finish Adler-32 (a = (1 + S0) mod 65521, b = (n + n S0 - S1) mod 65521).
//   3 emit    one wave per row walks the row again; an end lane ORs its tokens into the wave's LDS bit buffer at the wave scan of the
//             bit counts (LDS atomic OR: neighbouring tokens share words), then the wave stores the row's bytes at its offset.
// Encoding twice against encoding once into a worst-case-strided scratch and compacting: the scratch would be (9 (W + 1) / 8 + 8) bytes
// per row (37 MB for 36 planes of 720 x 1280) to be allocated, and its compaction is a launch that reads and writes every byte
// again; the second walk reads planes that the first one left in the cache and the count pass needs no LDS at all.
//
// Everything read back from the workspace is clamped before it addresses anything; a row is stored only where it lies inside out_cap.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocpg_hip.h"

namespace {

typedef unsigned long long u64;

constexpr int WMAX = 4096;                                   // widest row served: sizes the per-wave LDS bit buffer
constexpr int NT = 256;                                      // threads per workgroup: 4 waves = 4 rows
constexpr int WAVES = NT / 64;
constexpr int MAX_ROWS = 1 << 22;                            // N * H
constexpr int NT2 = 256;                                     // threads of the scan workgroup

// bytes of a coded row: header 3 bits, at most 9 bits per filtered byte (a match of >= 3 bytes costs at most 18), end-of-block 7,
// stored header 3, padding, 4 bytes; + 2 for the final block behind a plane's last row
__host__ __device__ inline int row_bytes_max(int W) { return (9 * (W + 1) + 13 + 7) / 8 + 4 + 2; }
constexpr int ROW_WORDS = ((9 * (WMAX + 1) + 13 + 7) / 8 + 4 + 2 + 3) / 4 + 1;   // + 1: the high half of a 64-bit OR

struct Workspace {
  long long* rowoff;       // [R] byte offset of the row in the output
  u64* s1;                 // [R] sum(p * d) over the row's filtered positions
  int* rowlen;             // [R] bytes of the coded row (the plane's last row: + 2)
  unsigned* s0;            // [R] sum(d)
};

__host__ __device__ inline Workspace carve(void* p, long long R) {
  Workspace w;
  w.rowoff = (long long*)p;
  w.s1 = (u64*)(w.rowoff + R);
  w.rowlen = (int*)(w.s1 + R);
  w.s0 = (unsigned*)(w.rowlen + R);
  return w;
}

__device__ __forceinline__ int lit_bits(int v) { return v < 144 ? 8 : 9; }

// length 3..258 -> bits of its symbol + extra bits + the 5-bit distance
__device__ __forceinline__ int match_bits(int len) {
  const int l = len - 3;
  if (l < 8) return 7 + 5;
  if (len == 258) return 8 + 5;
  const int e = 29 - __clz(l);                               // msb(l) - 2
  const int sym = 257 + 4 * e + (l >> e);
  return (sym < 280 ? 7 : 8) + e + 5;
}

__device__ __forceinline__ int run_bits(int v, int n) {
  const int lb = lit_bits(v), r = n - 1, k = r / 258, rem = r - k * 258;
  return lb + 13 * k + (rem >= 3 ? match_bits(rem) : rem * lb);
}

// ORs `val` (at most 32 bits) into the bit buffer at bit `pos`
__device__ __forceinline__ void put(unsigned* buf, unsigned pos, unsigned val) {
  const unsigned wi = pos >> 5;
  if (wi + 1 >= (unsigned)ROW_WORDS) return;                 // never taken: the buffer holds the longest row of WMAX
  const u64 v = (u64)val << (pos & 31);
  atomicOr(&buf[wi], (unsigned)v);
  if (v >> 32) atomicOr(&buf[wi + 1], (unsigned)(v >> 32));
}

__device__ __forceinline__ unsigned rev(unsigned code, int len) { return __brev(code) >> (32 - len); }

__device__ __forceinline__ unsigned put_literal(unsigned* buf, unsigned pos, int v) {
  if (v < 144) {
    put(buf, pos, rev(0x30 + v, 8));
    return pos + 8;
  }
  put(buf, pos, rev(0x190 + (v - 144), 9));
  return pos + 9;
}

__device__ __forceinline__ unsigned put_match(unsigned* buf, unsigned pos, int len) {
  const int l = len - 3;
  int sym, e = 0;
  if (l < 8) sym = 257 + l;
  else if (len == 258) sym = 285;
  else {
    e = 29 - __clz(l);
    sym = 257 + 4 * e + (l >> e);
  }
  const int sb = sym < 280 ? 7 : 8;
  const unsigned code = sym < 280 ? rev(sym - 256, 7) : rev(0xC0 + (sym - 280), 8);
  put(buf, pos, code | ((unsigned)(l & ((1 << e) - 1)) << sb));      // the distance code is five zero bits
  return pos + sb + e + 5;
}

__device__ __forceinline__ void put_run(unsigned* buf, unsigned pos, int v, int n) {
  pos = put_literal(buf, pos, v);
  int r = n - 1;
  for (; r >= 258; r -= 258) pos = put_match(buf, pos, 258);
  if (r >= 3) put_match(buf, pos, r);
  else
    for (; r > 0; --r) pos = put_literal(buf, pos, v);
}

// One wave walks one row.  -> the bit position behind the row's last token (the 3 header bits included).  EMIT: tokens are ORed into
// buf (zeroed, this wave's); otherwise s0 / s1 are the lane's partial sums.
template <bool EMIT>
__device__ __forceinline__ unsigned walk_row(const unsigned char* __restrict__ row, int W, unsigned* buf, unsigned& s0, unsigned& s1) {
  const int lane = threadIdx.x & 63;
  const int n = W + 1;
  auto load = [&](int p) -> int { return p == 0 ? 0 : (p < n ? (int)row[p - 1] : -1); };
  unsigned bitpos = 3;
  int prev_end = -1;
  int cur = load(lane);
#pragma unroll 1
  for (int g = 0; g < n; g += 64) {
    const int p = g + lane;
    const int nxt = load(p + 64);
    int succ = __shfl_down(cur, 1);
    const int head = __shfl(nxt, 0);
    if (lane == 63) succ = head;
    const bool valid = p < n;
    const bool is_end = valid && succ != cur;
    const u64 ends = __ballot(is_end);
    const u64 below = ends & ((1ull << lane) - 1ull);
    const int pe = below ? g + 63 - __clzll((long long)below) : prev_end;
    const int len = p - pe;
    const int nb = is_end ? run_bits(cur, len) : 0;
    int inc = nb;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    if constexpr (EMIT) {
      if (is_end) put_run(buf, bitpos + (unsigned)(inc - nb), cur, len);
    } else if (valid) {
      s0 += (unsigned)cur;
      s1 += (unsigned)p * (unsigned)cur;                     // per lane at most 65 * 4096 * 255 < 2^27
    }
    bitpos += (unsigned)__shfl(inc, 63);
    if (ends) prev_end = g + 63 - __clzll((long long)ends);
    cur = nxt;
  }
  return bitpos;
}

// tokens end at bit `bitpos`: end-of-block (7) and the stored header (3) follow, then padding -> the first byte of 00 00 FF FF
__device__ __forceinline__ int stored_at(unsigned bitpos) { return (int)((bitpos + 10 + 7) >> 3); }

__global__ __launch_bounds__(NT) void png_count(const unsigned char* __restrict__ planes, int H, int W, int R, Workspace ws) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (r >= R) return;
  unsigned s0 = 0, s1 = 0;
  const unsigned bitpos = walk_row<false>(planes + (long long)r * W, W, nullptr, s0, s1);
  u64 a = s0, b = s1;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    a += __shfl_xor(a, d);
    b += __shfl_xor(b, d);
  }
  if (lane == 0) {
    ws.rowlen[r] = stored_at(bitpos) + 4 + ((r % H) == H - 1 ? 2 : 0);
    ws.s0[r] = (unsigned)a;
    ws.s1[r] = b;
  }
}

__device__ __forceinline__ u64 block_sum(u64 v, u64* s_red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  __syncthreads();                                           // the previous use of s_red is over
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  u64 t = 0;
#pragma unroll
  for (int i = 0; i < NT2 / 64; ++i) t += s_red[i];
  return t;
}

__global__ __launch_bounds__(NT2) void png_scan(int H, int W, Workspace ws, long long* __restrict__ totals) {
  __shared__ u64 s_red[NT2 / 64];
  __shared__ int s_tot[NT2 / 64];
  const int m = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lmax = row_bytes_max(W);
  auto len_of = [&](long long r) -> int {
    const int l = ws.rowlen[r];
    return l < 0 ? 0 : (l > lmax ? lmax : l);
  };
  const long long first = (long long)m * H;
  u64 before = 0;
  for (long long r = threadIdx.x; r < first; r += NT2) before += (u64)len_of(r);
  before = block_sum(before, s_red);
  u64 a = 0, b = 0;
  long long carry = 0;
  for (int y0 = 0; y0 < H; y0 += NT2) {
    const int y = y0 + threadIdx.x;
    int l = 0;
    if (y < H) {
      l = len_of(first + y);
      const u64 s0 = ws.s0[first + y];
      a += s0;
      b += (u64)y * (u64)(W + 1) * s0 + ws.s1[first + y];
    }
    int inc = l;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    __syncthreads();                                         // the previous block's totals have been read
    if (lane == 63) s_tot[wave] = inc;
    __syncthreads();
    int pre = 0, all = 0;
#pragma unroll
    for (int i = 0; i < NT2 / 64; ++i) {
      pre += i < wave ? s_tot[i] : 0;
      all += s_tot[i];
    }
    if (y < H) ws.rowoff[first + y] = (long long)before + carry + pre + (inc - l);
    carry += all;
  }
  a = block_sum(a, s_red);
  b = block_sum(b, s_red);
  if (threadIdx.x == 0) {
    totals[3 * m] = carry;
    totals[3 * m + 1] = (long long)a;
    totals[3 * m + 2] = (long long)b;
  }
}

__global__ __launch_bounds__(NT) void png_emit(const unsigned char* __restrict__ planes, int H, int W, int R, Workspace ws,
                                               unsigned char* __restrict__ out, long long out_cap) {
  __shared__ unsigned s_buf[WAVES][ROW_WORDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * WAVES + wave;
  const bool live = r < R;                                   // every wave reaches both barriers
  unsigned* buf = s_buf[wave];
  int len = 0;
  long long off = 0;
  if (live) {
    len = ws.rowlen[r];
    const int lmax = row_bytes_max(W);
    len = len < 0 ? 0 : (len > lmax ? lmax : len);
    off = ws.rowoff[r];
    const int nw = (len + 3) / 4 + 1;                        // <= ROW_WORDS: len <= row_bytes_max(WMAX)
    for (int i = lane; i < nw; i += 64) buf[i] = 0;
  }
  __syncthreads();
  int made = 0;
  if (live) {
    unsigned s0 = 0, s1 = 0;
    const unsigned bitpos = walk_row<true>(planes + (long long)r * W, W, buf, s0, s1);
    if (lane == 0) {
      put(buf, 0, 2u);                                       // BFINAL = 0, BTYPE = 01: the bits 0, 1, 0
      const int at = stored_at(bitpos);
      put(buf, (unsigned)(at + 2) * 8u, 0xFFFFu);            // 00 00 FF FF
      if ((r % H) == H - 1) put(buf, (unsigned)(at + 4) * 8u, 0x03u);           // the final block: 03 00
    }
    made = stored_at(bitpos) + 4 + ((r % H) == H - 1 ? 2 : 0);
  }
  __syncthreads();
  if (live && made == len && off >= 0 && off + len <= out_cap) {
    unsigned char* o = out + off;
    for (int i = lane; i < len; i += 64) o[i] = (unsigned char)(buf[i >> 2] >> (8 * (i & 3)));
  }
}

int check_shape(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return -1006;
  if (W > WMAX) return -2701;
  if (N > 65535 || H > 65535 || (long long)N * H > MAX_ROWS) return -2702;
  return 0;
}

}  // namespace

extern "C" int ocpg_png_rle_count(const unsigned char* planes, int N, int H, int W, void* workspace, long long* totals, void* stream) {
  const int rc = check_shape(N, H, W);
  if (rc) return rc;
  if (!planes) return -1001;
  if (!workspace || ((uintptr_t)workspace & 7)) return -2703;
  if (!totals || ((uintptr_t)totals & 7)) return -2704;
  const int R = N * H;
  const Workspace ws = carve(workspace, R);
  hipStream_t st = (hipStream_t)stream;
  png_count<<<(unsigned)((R + WAVES - 1) / WAVES), NT, 0, st>>>(planes, H, W, R, ws);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return -(int)e;
  png_scan<<<(unsigned)N, NT2, 0, st>>>(H, W, ws, totals);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

extern "C" int ocpg_png_rle_emit(const unsigned char* planes, int N, int H, int W, void* workspace, const long long* totals_host,
                                 unsigned char* out, long long out_cap, void* stream) {
  const int rc = check_shape(N, H, W);
  if (rc) return rc;
  if (!planes) return -1001;
  if (!workspace || ((uintptr_t)workspace & 7)) return -2703;
  if (!totals_host) return -2705;
  long long need = 0;
  for (int m = 0; m < N; ++m) {
    const long long b = totals_host[3 * (long long)m];
    if (b < 0 || b > (long long)H * row_bytes_max(W)) return -2705;
    need += b;
  }
  if (!out || out_cap <= 0 || need > out_cap) return -2706;
  const int R = N * H;
  const Workspace ws = carve(workspace, R);
  png_emit<<<(unsigned)((R + WAVES - 1) / WAVES), NT, 0, (hipStream_t)stream>>>(planes, H, W, R, ws, out, out_cap);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
