// The kernel of csrc/conv3x3_mfma.hip, included there once per 16-bit storage type with
//   CONV3X3_KERNEL  the kernel's name (conv3x3_mfma: bf16, conv3x3_mfma_f16: fp16)
//   CONV3X3_ELEM    its element trait (Bf16 / Fp16: storage type, MFMA opcode, final narrowing)
// defined: ONE body.  (A __device__ body inlined into per-type __global__ wrappers was tried first: it changed the register allocation
// of the bf16 instantiations -- the geometry struct then reaches the lambdas through a copy -- and they must not move.)
// SPLITK (64-column tiles only; round 4): blockIdx.z takes a contiguous range of the 64-channel chunks of K and the tile leaves as fp32
// partial sums part[z][row][col] (y = that buffer; no affine / ReLU: ocpg_splitk_reduce finishes) -- for convolutions whose GEMM has few
// rows and a long K: the neck's stride-2 level (models/ocpg.py:119-123: 600 output pixels x 256 channels, K = 18 432 = 288 steps on 40
// workgroups without the split).
// BTR (input gradient only; round 4): the weight operand is the convolution's OWN weight [Cout_conv, 3, 3, Cin_conv] (no per-step
// transposed copy: 30 ATen transposes, 0.26 ms per step).  For the input gradient the GEMM's K axis is (tap, output channel) and its N axis
// the input channel, so a K step's B tile is 64 weight ROWS (k) x BN contiguous input channels (n): it is staged as it lies, [k][n], and
// the MFMA fragments -- 8 consecutive k of one n -- are read TRANSPOSED with gfx950's ds_read_b64_tr_b16 (per 16-lane group a 4-row x
// 16-column block, delivered column-major: lane 4q + p supplies row q, columns 4p..4p+3, lane i receives column i of the 4 rows).
// COLS (forward only): the launch also writes the patch matrix (cols).  A template parameter, not a run-time test of the pointer: the
// forward without it keeps no patch-matrix column and no store address live through the K loop and fits three workgroups per CU.
// CLS (own-weight input gradient of a stride-2 convolution): a 64-row tile holds input pixels of ONE parity class (y & 1, x & 1), and its
// K loop walks only the taps that reach that class (4, 2, 2 or 1 of the 9; the other taps' rows are all zero padding).  blockIdx.x runs
// over the classes' tile ranges (g.ctile), the heavy class first: (1,1), (0,1), (1,0), (0,0).  The non-zero products of an output element
// and their order are those of the nine-tap walk, so the result is bit-identical for finite operands.
template <bool DGRAD, int BN, bool SPLITK = false, bool BTR = false, bool COLS = false, bool CLS = false>
__global__ __launch_bounds__(NT) void CONV3X3_KERNEL(const CONV3X3_ELEM::T* __restrict__ x, const CONV3X3_ELEM::T* __restrict__ w,
                                                     const float* __restrict__ scale, const float* __restrict__ bias, int relu, ConvGeom g,
                                                     CONV3X3_ELEM::T* __restrict__ y, CONV3X3_ELEM::T* __restrict__ cols,
                                                     const CONV3X3_ELEM::T* __restrict__ mask = nullptr) {
  using E = CONV3X3_ELEM;
  using T = E::T;
  // mask (round 4; same [row][column] layout as y, or null): an element is kept only where mask > 0 -- the input-gradient launch then ALSO
  // does the frozen-BN + ReLU backward of the layer in front (gz = gx * scale[c] * [y_prev > 0], csrc/bn_act.hip's job until round 3)
  static_assert(!SPLITK || BN == 64, "the split-K epilogue is the 64-column one");
  static_assert(!BTR || DGRAD, "the untransposed weight operand is the input gradient's");
  static_assert(!COLS || !DGRAD, "the patch matrix is the forward's");
  static_assert(!CLS || (BTR && !SPLITK), "parity-class tiles are the own-weight input gradient's");
  constexpr int BROW = BN + 8;           // BTR: LDS row of the [k][n] B tile (bf16 elements; 16-byte aligned, rows 4 banks apart)
  constexpr int BSEG = BN / 8;           // BTR: 16-byte segments per staged k row
  static_assert(BK * BROW <= BN * LDS_ROW, "the [k][n] image fits the [n][k] one's buffer");
  constexpr int B_L = BN / ROWS_PER_PASS, NJ = BN / 64, WN = BN / 2;      // a wave's tile: 32 rows x WN columns = NJ MFMA tiles
  // 64-column tiles: the four waves split the K STEP instead of the tile (wave w takes the 16-wide slice w of every 64-wide step and
  // accumulates the whole 64 x 64 tile = 2 x 2 MFMA tiles): two A and two B fragments feed four MFMAs, where a 32 x 32 wave tile reads
  // two fragments per MFMA -- the kernel was bound by LDS read bandwidth (32 KB of fragment reads per workgroup and K step against
  // 16 KB of global data), not by the matrix cores or HBM.  The four partial tiles are summed through LDS once, after the K loop.
  constexpr bool KSPLIT = BN == 64;
  constexpr int NACC = KSPLIT ? 4 : NJ;
  __shared__ __attribute__((aligned(16))) short smem[2 * BM * LDS_ROW + 2 * BN * LDS_ROW];
  short (*As)[BM * LDS_ROW] = reinterpret_cast<short (*)[BM * LDS_ROW]>(smem);
  short (*Bs)[BN * LDS_ROW] = reinterpret_cast<short (*)[BN * LDS_ROW]>(smem + 2 * BM * LDS_ROW);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;                 // wave tile: rows wm*32.., cols wn*64..
  // CLS: class k of this tile, its parity (cpy, cpx), extents and tap list (4 bits per tap, ascending); m0 counts pixels WITHIN the class
  int cpy = 0, cpx = 0, ntaps = 9;
  unsigned taplist = 0;
  int tile = blockIdx.x;
  if constexpr (CLS) {
    const int k = (tile >= g.ctile[0]) + (tile >= g.ctile[1]) + (tile >= g.ctile[2]);
    if (k > 0) tile -= g.ctile[k - 1];
    cpy = (k & 1) ^ 1;
    cpx = k < 2;
    ntaps = k == 0 ? 4 : k == 3 ? 1 : 2;
    taplist = k == 0 ? 0x8620u : k == 1 ? 0x53u : k == 2 ? 0x71u : 0x4u;      // ky = 1 - cpy (+2 when cpy), kx = 1 - cpx (+2 when cpx)
  }
  const int rH = CLS ? (g.H - cpy + 1) / 2 : g.H, rW = CLS ? (g.W - cpx + 1) / 2 : g.W;      // the map the tile's rows enumerate
  const long long rM = CLS ? (long long)g.N * rH * rW : g.M;
  const long long m0 = (long long)tile * BM;
  const int n0 = blockIdx.y * BN;
  // ---- staging identity: 16-B segment sseg of rows srow + i * ROWS_PER_PASS (A: i < A_L, B: i < B_L)
  const int srow = tid / SEGS, sseg = tid % SEGS;
  int pn[A_L], py[A_L], px[A_L];
  bool row_ok[A_L];
  {
    const int hw = rH * rW;
#pragma unroll
    for (int i = 0; i < A_L; ++i) {
      const long long mrow = m0 + srow + i * ROWS_PER_PASS;
      row_ok[i] = mrow < rM;
      const long long mr = row_ok[i] ? mrow : 0;
      pn[i] = (int)(mr / hw);
      const int r = (int)(mr - (long long)pn[i] * hw);
      py[i] = r / rW;
      px[i] = r - py[i] * rW;
      if constexpr (CLS) { py[i] = 2 * py[i] + cpy; px[i] = 2 * px[i] + cpx; }
    }
  }
  const int C = g.C, ksteps_per_tap = C / BK;
  const int cps = SPLITK ? ksteps_per_tap / (int)gridDim.z : ksteps_per_tap;      // 64-channel chunks of this workgroup (the host made it divide)
  const int c_lo = SPLITK ? (int)blockIdx.z * cps : 0, c_hi = c_lo + cps;
  const int ksteps = (CLS ? ntaps : 9) * cps;
  const long long wrow_stride = 9LL * C;                   // elements between consecutive GEMM-N rows of the weight operand
  const T* wp[B_L];                                        // rows past Cout are clamped: their columns are never stored
#pragma unroll
  for (int i = 0; i < B_L; ++i) {
    if constexpr (BTR) {                                     // segment e of the [64 k][BN n] tile: k row e / BSEG, columns 8 (e % BSEG)..
      const int e = tid + i * NT, kr = e / BSEG, ns = e % BSEG;
      wp[i] = w + (long long)kr * (9LL * g.Cout) + min(n0 + ns * 8, g.Cout - 8);      // (a weight row is 9 * Cin_conv long; Cin_conv = g.Cout here)
    } else {
      wp[i] = w + (long long)min(n0 + srow + i * ROWS_PER_PASS, g.Cout - 1) * wrow_stride + sseg * 8;
    }
  }

  // NSETS register sets: the loads of K step s + NSETS + 1 are issued while step s computes, so a load has NSETS MFMA phases
  // (not a fraction of one) to come back -- at ~1 workgroup per CU (300 workgroups for ResNet-101's layer3 shape) nothing
  // else hides it.  Loads are unconditional (clamped address, zeroed at park time): a load inside a branch gets its own
  // s_waitcnt and serialises the batch.
  struct Regs { uint4 a[A_L], b[B_L]; unsigned z; int coff; };     // z bit i: A row i of this set is zero padding; coff (COLS only): its column in the patch matrix (-1: past the end)
  Regs S0, S1;
  int f_tap = 0, f_c = c_lo;                               // K position of the NEXT fetch (fetches are issued in K order)
  // Fetches are UNCONDITIONAL, also past the last K step (clamped to the last tap: valid memory, never parked into a buffer that is
  // read): with `if (s + 3 < ksteps) fetch(...)` the compiler has to assume the path on which the fetch did not happen, on which the
  // register set about to be parked holds the MOST RECENT loads -- it then waits with vmcnt(3..0), i.e. also for the four loads issued
  // one step ago, and the two-step prefetch distance silently became one (seen in the ISA; 1 830 cycles per K step and wave).
  auto fetch = [&](Regs& R) {
    uint4 (&a)[A_L] = R.a; uint4 (&bq)[B_L] = R.b; unsigned& z = R.z;
    // K order: the nine taps of one 64-channel chunk, then the next chunk -- consecutive steps then read the SAME 128-byte lines of
    // neighbouring pixels (a tap shifts the tile by one pixel or one row), which the L1 still holds; tap-major order re-read every
    // line from L2 nine times, and the launch is bound by the CU's L1-miss bandwidth (10 B/cycle with one workgroup per CU, 19 with three)
    const int tap = CLS ? (int)((taplist >> (4 * f_tap)) & 15u) : f_tap, fc = min(f_c, c_hi - 1);      // f_tap < ntaps also past the end
    const int ky = (tap * 11) >> 5, kx = tap - ky * 3;      // tap / 3 for tap < 9
    const int c0 = fc * BK + sseg * 8;
    if constexpr (COLS) R.coff = f_c < c_hi ? tap * C + c0 : -1;
    z = 0;
#pragma unroll
    for (int i = 0; i < A_L; ++i) {
      int ys = 0, xs = 0;
      const bool ok = row_ok[i] && tap_source<DGRAD>(g, py[i], px[i], ky, kx, ys, xs);
      if (!ok) { ys = 0; xs = 0; z |= 1u << i; }
      a[i] = *reinterpret_cast<const uint4*>(x + (((long long)pn[i] * g.Hs + ys) * g.Ws + xs) * C + c0);
    }
    const long long woff = BTR ? (long long)fc * BK * (9LL * g.Cout) + (long long)tap * g.Cout : (long long)tap * C + fc * BK;
#pragma unroll
    for (int i = 0; i < B_L; ++i) bq[i] = *reinterpret_cast<const uint4*>(wp[i] + woff);
    if (++f_tap == (CLS ? ntaps : 9)) { f_tap = 0; ++f_c; }
  };
  auto park = [&](int buf, const Regs& R) {
    const uint4 (&a)[A_L] = R.a; const uint4 (&bq)[B_L] = R.b; const unsigned z = R.z;
#pragma unroll
    for (int i = 0; i < A_L; ++i)
      *reinterpret_cast<uint4*>(&As[buf][(srow + i * ROWS_PER_PASS) * LDS_ROW + sseg * 8]) = ((z >> i) & 1u) ? make_uint4(0u, 0u, 0u, 0u) : a[i];
#pragma unroll
    for (int i = 0; i < B_L; ++i) {
      if constexpr (BTR) {
        const int e = tid + i * NT;
        *reinterpret_cast<uint4*>(&Bs[buf][(e / BSEG) * BROW + (e % BSEG) * 8]) = bq[i];
      } else {
        *reinterpret_cast<uint4*>(&Bs[buf][(srow + i * ROWS_PER_PASS) * LDS_ROW + sseg * 8]) = bq[i];
      }
    }
    if constexpr (COLS) {
      // the gathered A tiles ARE the rows of the patch (im2col) matrix the weight gradient contracts with: the column-0 workgroups
      // write them out on the way (16 bytes per thread and row) and the backward needs no im2col pass
      if (blockIdx.y == 0 && R.coff >= 0) {
#pragma unroll
        for (int i = 0; i < A_L; ++i)
          if (row_ok[i])
            *reinterpret_cast<uint4*>(cols + (m0 + srow + i * ROWS_PER_PASS) * (9LL * C) + R.coff) = ((z >> i) & 1u) ? make_uint4(0u, 0u, 0u, 0u) : a[i];
      }
    }
  };

  f32x16 acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  const int fr = lane & 31, fh = lane >> 5;                // fragment row / k-half of this lane
  // BTR: fragment (8 consecutive k from k0 + 8 fh, column ncol0 + fr) out of the [k][n] tile by two transposing reads
  auto btr = [&](int buf, int k0, int ncol0) -> bf16x8 {
    typedef short s4 __attribute__((ext_vector_type(4)));
    const int li = lane & 15, grp = lane >> 4;
    const short* p = &Bs[buf][(k0 + 8 * fh + (li >> 2)) * BROW + ncol0 + 16 * (grp & 1) + 4 * (li & 3)];
    const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)p);
    const s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(p + 4 * BROW));
    bf16x8 r;
    r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3]; r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
    return r;
  };
  auto compute = [&](int buf) {
    if constexpr (KSPLIT) {
      static_assert(BK / 16 == NT / 64, "one 16-wide K slice per wave");
      const int ko = wave * 16 + fh * 8;
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(&As[buf][fr * LDS_ROW + ko]);
      const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(&As[buf][(32 + fr) * LDS_ROW + ko]);
      bf16x8 b0, b1;
      if constexpr (BTR) {
        b0 = btr(buf, wave * 16, 0);
        b1 = btr(buf, wave * 16, 32);
      } else {
        b0 = *reinterpret_cast<const bf16x8*>(&Bs[buf][fr * LDS_ROW + ko]);
        b1 = *reinterpret_cast<const bf16x8*>(&Bs[buf][(32 + fr) * LDS_ROW + ko]);
      }
      acc[0] = E::mfma(a0, b0, acc[0]);
      acc[1] = E::mfma(a0, b1, acc[1]);
      acc[2] = E::mfma(a1, b0, acc[2]);
      acc[3] = E::mfma(a1, b1, acc[3]);
      return;
    }
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(&As[buf][(wm * 32 + fr) * LDS_ROW + kk * 16 + fh * 8]);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        bf16x8 b;
        if constexpr (BTR) b = btr(buf, kk * 16, wn * WN + j * 32);
        else b = *reinterpret_cast<const bf16x8*>(&Bs[buf][(wn * WN + j * 32 + fr) * LDS_ROW + kk * 16 + fh * 8]);
        acc[j] = E::mfma(a, b, acc[j]);
      }
    }
  };
  // Three register sets rotate (step s waits in set s % 3), two LDS buffers alternate (step s is parked into buffer s % 2);
  // ksteps = 9 * C / BK is a multiple of 3 (CLS: ntaps * C / BK need not be: a step past ksteps parks a clamped fetch into a buffer
  // nothing reads and skips its compute).  A load has three compute phases to come back: one workgroup alone on a CU measured
  // 0.65 us per K step with two sets (= half a load's round trip under load), and the layer3 launch has only 2.3 workgroups per CU.
  static_assert(NSETS == 3, "the k loop below is written for three register sets");
  Regs S2;
  fetch(S0);
  fetch(S1);
  fetch(S2);
  park(0, S0);
  fetch(S0);                                               // step 3
  __syncthreads();
  auto step = [&](int s_, Regs& nxt) {                     // nxt holds step s_ + 1
    park((s_ & 1) ^ 1, nxt);                               // that buffer was last read in step s_ - 1 (barrier since); past the end: unread
    fetch(nxt);                                            // step s_ + 4 (past the end: a clamped, unused load)
    if (s_ < ksteps) compute(s_ & 1);
    __syncthreads();
  };
  for (int ks = 0; ks < ksteps; ks += 3) {
    step(ks, S1);
    step(ks + 1, S2);
    step(ks + 2, S0);
  }
  // CLS: tile row -> row of dx / mask (-1: past the class's last pixel), through LDS behind the two tile images of the reduction below
  long long* rowmap = reinterpret_cast<long long*>(smem + 4 * 4096);
  static_assert(!CLS || sizeof(smem) >= 2 * 4096 * sizeof(float) + BM * sizeof(long long), "the row map lies behind the tile images");
  if constexpr (CLS) {
    if (tid < BM) {
      const long long q = m0 + tid;
      const int hw = rH * rW, qn = (int)(q / hw), r = (int)(q - (long long)qn * hw), qy = r / rW, qx = r - qy * rW;
      rowmap[tid] = q < rM ? ((long long)qn * g.H + 2 * qy + cpy) * g.W + 2 * qx + cpx : -1;
    }
    if constexpr (!KSPLIT) __syncthreads();      // (the 64-column form has its reduction's barriers in between)
  }
  if constexpr (KSPLIT) {
    // ---- sum the four waves' partial 64 x 64 tiles through LDS (the K loop ended with a barrier: the staging buffers are free).
    // A tile image is [MFMA tile t = 2 * (row / 32) + col / 32][register r][lane]: 4096 floats, conflict-free for its writer.
    float* red = reinterpret_cast<float*>(smem);
    static_assert(sizeof(smem) >= 2 * 4096 * sizeof(float), "two tile images");
    auto put = [&](float* d) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) d[(t * 16 + r) * 64 + lane] = acc[t][r];
    };
    auto add = [&](const float* d) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] += d[(t * 16 + r) * 64 + lane];
    };
    if (wave >= 2) put(red + (wave - 2) * 4096);
    __syncthreads();
    if (wave < 2) add(red + wave * 4096);
    __syncthreads();
    if (wave == 1) put(red + 4096);
    __syncthreads();
    if (wave == 0) { add(red + 4096); put(red); }
    __syncthreads();
    // ---- epilogue by all 256 threads: thread = (tile row m, 16 consecutive columns) -> one 32-byte store
    const int m = tid >> 2, nq = (tid & 3) * 16;
    const long long row = CLS ? rowmap[m] : m0 + m;
    if (CLS ? row >= 0 : row < g.M) {
      const int r = (m & 3) + 4 * ((m & 31) >> 3), h = ((m & 31) >> 2) & 1, t0 = (m >> 5) * 2 + (nq >> 5);
      const float* src = red + (t0 * 16 + r) * 64 + (nq & 31) + 32 * h;
      const int col0 = n0 + nq;
      if constexpr (SPLITK) {                                                   // fp32 partial sums of this K range, 64 bytes per thread
        float* dst = reinterpret_cast<float*>(y) + ((long long)blockIdx.z * g.M + row) * g.Cout + col0;
        if (col0 + 16 <= g.Cout && (g.Cout & 3) == 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q) reinterpret_cast<float4*>(dst)[q] = make_float4(src[4 * q], src[4 * q + 1], src[4 * q + 2], src[4 * q + 3]);
        } else {
          for (int j = 0; j < 16 && col0 + j < g.Cout; ++j) dst[j] = src[j];
        }
        return;
      }
      short o[16];
      float sc[16], bi[16];
      const bool full = col0 + 16 <= g.Cout;
      if (full) {                                                             // 16 consecutive floats each: 4 + 4 vector loads, issued together
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 a = scale ? reinterpret_cast<const float4*>(scale + col0)[q] : make_float4(1.f, 1.f, 1.f, 1.f);
          const float4 b = bias ? reinterpret_cast<const float4*>(bias + col0)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
          sc[4 * q] = a.x, sc[4 * q + 1] = a.y, sc[4 * q + 2] = a.z, sc[4 * q + 3] = a.w;
          bi[4 * q] = b.x, bi[4 * q + 1] = b.y, bi[4 * q + 2] = b.z, bi[4 * q + 3] = b.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int col = min(col0 + j, g.Cout - 1);
          sc[j] = scale ? scale[col] : 1.f;
          bi[j] = bias ? bias[col] : 0.f;
        }
      }
      bool keep[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) keep[j] = true;
      if (mask) {
        const T* mk = mask + row * g.Cout + col0;
        if (full && (g.Cout & 7) == 0) {
          const bf16x8 lo = *reinterpret_cast<const bf16x8*>(mk), hi = *reinterpret_cast<const bf16x8*>(mk + 8);
#pragma unroll
          for (int j = 0; j < 8; ++j) { keep[j] = lo[j] > 0; keep[8 + j] = hi[j] > 0; }      // bf16 / fp16 > 0 <=> its bits as a signed short > 0
        } else {      // static indices into keep[] / o[]: a run-time j put o[] into scratch
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if (col0 + j < g.Cout) keep[j] = reinterpret_cast<const short*>(mk)[j] > 0;
        }
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        float v = src[j] * sc[j] + bi[j];                                     // frozen-BN affine / conv bias in the epilogue
        if (relu) v = fmaxf(v, 0.f);
        if (!keep[j]) v = 0.f;
        o[j] = (short)E::bits(v);
      }
      T* dst = y + row * g.Cout + col0;
      if (col0 + 16 <= g.Cout && (g.Cout & 7) == 0) {
        bf16x8 lo, hi;
#pragma unroll
        for (int j = 0; j < 8; ++j) { lo[j] = o[j]; hi[j] = o[8 + j]; }
        *reinterpret_cast<bf16x8*>(dst) = lo;
        *reinterpret_cast<bf16x8*>(dst + 8) = hi;
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (col0 + j < g.Cout) reinterpret_cast<short*>(dst)[j] = o[j];
      }
    }
    return;
  }
  // ---- epilogue: C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = n0 + wn * WN + j * 32 + (lane & 31);
    if (col >= g.Cout) continue;
    const float sv = scale ? scale[col] : 1.f, bv = bias ? bias[col] : 0.f;      // frozen-BN affine / conv bias in the epilogue
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      const long long row = CLS ? rowmap[m] : m0 + m;
      float v = acc[j][r] * sv + bv;
      if (relu) v = fmaxf(v, 0.f);
      if (CLS ? row >= 0 : row < g.M) {
        if (mask && !(reinterpret_cast<const short*>(mask)[row * g.Cout + col] > 0)) v = 0.f;
        y[row * g.Cout + col] = E::narrow(v);
      }
    }
  }
}
