// The body of the split-bf16 LDS-DMA GEMM kernels, as TEXT: included inside a __global__ function that provides
//   template / constexpr values  WM, WN, TM, TN, UP2, RELU, KXK, NS, P, PRE, D2S, K16
//   variables                    p (const ConvArgs, the KERNEL ARGUMENT itself), epi_vec, cb (D2S: columns per output-pixel block)
// gemm1x1s_launch.h (gemm1x1s_kernel: the convolution, PRE = D2S = false) and convt2x2s.hip (convt2x2s_kernel: the transposed 2x2 /
// stride-2 convolution -- the same main loop in front of the depth-to-space epilogue, D2S, with that layer's BatchNormalization
// prologue, PRE: scale | shift tables in LDS behind the operand stages, zero beyond K, applied in split8).
// Text rather than a device function on purpose: behind a function boundary (const ConvArgs& or by value, always inlined) hipcc
// no longer treats the fields of the kernel argument as wave-uniform everywhere -- the epilogues' scalar buffer offsets then
// go through readfirstlane loops (74-114 more instructions per kernel, measured on the instantiations of gemm1x1s_p1.hip).
// K16 (gemm1x1s_ext_launch.h: K x K with Cin % 16 == 0): the tap-major loop resolves (kh, kw, c0) per 16-channel HALF of the K-step
// instead of once per step, so a step may hold two taps; LDS layout, fragment reads, split and MFMA stream are those of KXK.
// Helpers: dma16, lds_rd, ... of lds_dma.h and split8, mfma_products, ... of split_bf16.h, which must be included first (with BK of
// gemm_family.h).
  static_assert(!(PRE && (KXK || UP2 || TM != 1)), "the BN prologue is built for the pipelined pointwise loop");
  static_assert(!(D2S && (KXK || UP2)), "the depth-to-space epilogue follows the plain pointwise main loop");
  static_assert(!K16 || KXK, "per-half taps are a form of the tap-major K x K loop");
  constexpr int NT = WM * WN * 64;
  constexpr bool PIPELINED = TM == 1;                    // software-pipelined K loop (below); else one chunk at a time
  constexpr int BM = WM * TM * 32;
  constexpr int BN = WN * TN * 32;
  constexpr int APASS = BM * 8 / NT;
  constexpr int BROWS = 4 * P * BN;                      // 16-byte units of the B stage: 4 k-groups x P parts x BN
  constexpr int BPASS = (BROWS + NT - 1) / NT;           // 16-byte units per thread (the last pass is partial)
  constexpr int STAGE = BM * BK + BROWS * 4;             // floats per stage
  constexpr int NPROD = nprod(P);
  static_assert(BM * 8 % NT == 0 && BROWS % 64 == 0, "tile/thread mismatch");

  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int li = lane & 31, lh = lane >> 5;

  const int M = p.N * p.OH * p.OW;
  const int tiles_n = (p.Cout + BN - 1) / BN;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int m0 = (tile / tiles_n) * BM;
  const int n0 = (tile % tiles_n) * BN;

  // ---- per-thread DMA sources: byte offsets into two buffer descriptors (activations, packed split weight)
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const auto rs_x = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.x), 0, (int)(((unsigned)(p.N * p.H * p.W - 1) * p.ldx + (unsigned)p.Cin) * 4u), 0x00020000);
  const auto rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0,
                                                      (int)((unsigned)p.Kp * p.Np * (2u * P)), 0x00020000);
  unsigned a_off[APASS];                                  // pointwise: (pixel * ldx + slot) * 4, fixed over K
  int a_slot[APASS];
  int a_pix[KXK ? APASS : 1], a_ih0[KXK ? APASS : 1], a_iw0[KXK ? APASS : 1];
#pragma unroll
  for (int ps = 0; ps < APASS; ++ps) {
    const int r = (tid >> 3) + ps * (NT / 8);
    int m = m0 + r;
    m = m < M ? m : M - 1;
    a_slot[ps] = ((tid & 7) ^ (r & 7)) * 4;
    if constexpr (KXK) {
      const int n = m / (p.OH * p.OW);
      const int rem = m - n * (p.OH * p.OW);
      const int oh = rem / p.OW, ow = rem - oh * p.OW;
      a_pix[ps] = n * p.H * p.W;
      a_ih0[ps] = oh * p.SH - p.PT;
      a_iw0[ps] = ow * p.SW - p.PL;
      a_off[ps] = 0;
    } else {
      a_off[ps] = ((unsigned)m * p.ldx + a_slot[ps]) * 4u;
    }
  }
  const int chunks_per_tap = KXK ? p.Cin / (K16 ? 16 : BK) : 1;
  const bool a_hi = a_slot[0] >= 16;                      // K16: the lane's slot lies in the second 16-k half (the same in every pass)
  // packed split weight: 16-byte unit (kg, part, n) at ((kg * P + part) * Np + n) * 16 bytes
  unsigned b_off[BPASS];
#pragma unroll
  for (int q = 0; q < BPASS; ++q) {
    const int idx = tid + q * NT;
    const int r = idx / BN;
    const int j = idx - r * BN;
    b_off[q] = r < 4 * P && n0 + j < p.Np ? ((unsigned)r * p.Np + n0 + j) * 16u : OOB;
  }
  const int b_step = 4 * P * p.Np * 16;                     // bytes per K-step in the packed weight

  auto issue = [&](int kt, int stage) {
    float* sA = smem + stage * STAGE;
    float* sB = sA + BM * BK;
    int kh = 0, kw = 0, c0 = 0;
    int kh1 = 0, kw1 = 0, c1 = 0;                           // K16: the second half's tap (wave-uniform like the first's)
    if constexpr (K16) {                                  // half k16 = 2 kt + h: tap k16 / (Cin / 16), c0 = (k16 mod (Cin / 16)) * 16
      const int tap = (2 * kt) / chunks_per_tap;
      c0 = (2 * kt - tap * chunks_per_tap) * 16;
      kh = tap / p.KW;
      kw = tap - kh * p.KW;
      const int tap1 = (2 * kt + 1) / chunks_per_tap;
      c1 = (2 * kt + 1 - tap1 * chunks_per_tap) * 16;
      kh1 = tap1 / p.KW;
      kw1 = tap1 - kh1 * p.KW;
    } else if constexpr (KXK) {
      const int tap = kt / chunks_per_tap;
      c0 = (kt - tap * chunks_per_tap) * BK;
      kh = tap / p.KW;
      kw = tap - kh * p.KW;
    }
#pragma unroll
    for (int ps = 0; ps < APASS; ++ps) {
      if constexpr (K16) {                                // padding taps and halves beyond K: out-of-range offset -> zeros
        const int ih = a_ih0[ps] + (a_hi ? kh1 : kh), iw = a_iw0[ps] + (a_hi ? kw1 : kw);
        const bool ok = (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W && (2 * kt + (a_hi ? 1 : 0)) * 16 < p.K;
        const unsigned off =
            ok ? ((unsigned)(a_pix[ps] + ih * p.W + iw) * p.ldx + (a_hi ? c1 : c0) + (a_slot[ps] & 15)) * 4u : OOB;
        dma16(rs_x, sA + (ps * NT + wave_u * 64) * 4, off, 0);
      } else if constexpr (KXK) {                         // padding taps: out-of-range offset -> zeros
        const int ih = a_ih0[ps] + kh, iw = a_iw0[ps] + kw;
        const bool ok = (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W && kt * BK < p.K;
        const unsigned off = ok ? ((unsigned)(a_pix[ps] + ih * p.W + iw) * p.ldx + c0 + a_slot[ps]) * 4u : OOB;
        dma16(rs_x, sA + (ps * NT + wave_u * 64) * 4, off, 0);
      } else {                                            // k >= K reads the next pixel (finite) or zeros: weights there are 0
        dma16(rs_x, sA + (ps * NT + wave_u * 64) * 4, a_off[ps], kt * BK * 4);
      }
    }
#pragma unroll
    for (int q = 0; q < BPASS; ++q)
      if ((q + 1) * NT <= BROWS || q * NT + wave_u * 64 < BROWS)     // whole waves: BROWS is a multiple of 64
        dma16(rs_w, sB + (q * NT + wave_u * 64) * 4, b_off[q], kt * b_step);
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = p.Kp / BK;
  // wait until at most `groups` of this wave's K-step DMA groups are outstanding (in-order counter; a wave that sits
  // out the partial last B pass issues one load less per group)
  const bool full_group = BPASS * NT <= BROWS || (BPASS - 1) * NT + wave_u * 64 < BROWS;
  auto wait_groups = [&](int groups) {
    constexpr int G = APASS + BPASS;
    if (groups == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (groups == 1) {
      if (full_group) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G - 1) : "memory");
    } else {
      if (full_group) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * G) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * G - 2) : "memory");
    }
  };
  issue(0, 0);
  if constexpr (!PIPELINED) {
    if constexpr (NS == 3) {
      if (nk > 1) issue(1, 1);
    }
    wait_groups(0);
  } else {                                            // pipelined loop: K-steps 1 .. NS-1 in flight from the start
    if (nk > 1) issue(1, 1);
    if constexpr (NS == 3) {
      if (nk > 2) issue(2, 2);
    }
    if constexpr (PRE) {            // scale | shift tables behind the stages, zero beyond K: a padded k slot becomes 0
      float* tab = smem + NS * STAGE;
      for (int i = tid; i < p.Kp; i += NT) {
        tab[i] = i < p.K ? p.pre_scale[i] : 0.f;
        tab[p.Kp + i] = i < p.K ? p.pre_shift[i] : 0.f;
      }
    }
    wait_groups(nk - 1 < NS - 1 ? nk - 1 : NS - 1);
  }
  __syncthreads();

  // ---- fragment read addresses (LDS byte offsets), stage 0.  A: row li of the wave's 32-row block, 8 consecutive k
  // of k-group (2c + lh) = slots 2(2c+lh), 2(2c+lh)+1 of the 128-byte row, XOR-swizzled with (row & 7) = (li & 7).
  const unsigned lds0 = (unsigned)(uintptr_t)(lptr_t)smem;
  unsigned a_base[2][TM][2];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        a_base[c][i][h] = lds0 + (unsigned)(((wm * TM + i) * 32 + li) * BK * 4 +
                                            (((2 * (2 * c + lh) + h) ^ (li & 7)) << 4));
  // B: unit ((2c + lh) * P + part) * BN + column
  const unsigned b_base = lds0 + (unsigned)(BM * BK * 4) + (unsigned)((lh * P * BN + wn * TN * 32 + li) * 16);

  EpiPrefetch<TM, TN> pre;
  if constexpr (!PIPELINED) {
  int cur = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if constexpr (!D2S) {
      if (kt == nk - 1) pre.template issue<WM, WN>(p, m0, n0, M, epi_vec);
    }
    const unsigned so = (unsigned)(cur * STAGE * 4);
    const unsigned bo = b_base + so;

    int nxt = cur + NS - 1;                           // stage that was read NS-1 ... 1 K-steps ago: free
    nxt = nxt >= NS ? nxt - NS : nxt;
    const bool more = kt + NS - 1 < nk;
    {
      // big per-wave tile (64 x 96): LDS fragment traffic per MFMA is what bounds this kernel (each wave re-reads its
      // B columns: 0.61 KB per MFMA at 32 x 96, 0.36 KB at 64 x 96), and 96 accumulators leave room for ONE chunk of
      // operands at a time -- no operand double buffering, the partner wave of the SIMD covers the read latency
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float4 ra1[TM][2], rb1[TN][P];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          ra1[i][0] = lds_rd<0>(a_base[c][i][0] + so);
          ra1[i][1] = lds_rd<0>(a_base[c][i][1] + so);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          rb1[j][0] = lds_rd<0>(bo + (unsigned)((2 * P * c) * BN * 16 + j * 512));
          if constexpr (P > 1) rb1[j][1] = lds_rd<0>(bo + (unsigned)((2 * P * c + 1) * BN * 16 + j * 512));
          if constexpr (P > 2) rb1[j][2] = lds_rd<0>(bo + (unsigned)((2 * P * c + 2) * BN * 16 + j * 512));
        }
        __builtin_amdgcn_sched_barrier(0);
        if (c == 0 && more) issue(kt + NS - 1, nxt);
        lgkm_wait();
        Frag<P> fa[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[i] = split8<RELU, P>(ra1[i][0], ra1[i][1]);
        bf16x8 fb[TN][P];
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int q = 0; q < P; ++q) fb[j][q] = as_bf(rb1[j][q]);
        mfma_products<TM, TN, 0, NPROD, P>(fa, fb, acc);
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    // K-step kt+1 must have landed: with three stages the loads just issued (K-step kt+2) may stay in flight
    // (in-order counter: "at most the loads of K-step kt+2 outstanding"; a wave that sat out the partial last B pass
    // issued one load less)
    if (NS == 3 && more) {
      if (BPASS * NT <= BROWS || (BPASS - 1) * NT + wave_u * 64 < BROWS)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(APASS + BPASS) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(APASS + BPASS - 1) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    cur = cur + 1 == NS ? 0 : cur + 1;
  }
  } else {
  // ---- software-pipelined loop (per-wave tiles of up to 5 MFMA tiles): the operands of chunk c+1 (16 k-values) are
  // read from LDS and split WHILE chunk c is multiplied, across K-steps too, so that between two MFMAs the wave only
  // ever issues what hides under them.  Measured before this structure (SQ counters, 64 x 32 x 32 x 576 -> 576): matrix
  // pipe 56 % busy; per wave and K-step 1152 cycles of MFMA and about as much again of exposed LDS round trips, split
  // arithmetic and barrier, which two uncoordinated work-groups per CU do not hide from each other (both waves of a
  // SIMD fall into step: the pipe is shared while both multiply and idle while both fetch).
  // One barrier per K-step, at the top of its SECOND chunk: by then every wave has finished reading stage kt-1 ... so
  // the DMA of K-step kt+NS-1 may overwrite it, and K-step kt+1 (issued NS-1 K-steps earlier) has landed.
  struct Ops { Frag<P> a[TM]; bf16x8 b[TN][P]; };
  Ops o0, o1;
  float4 ra[TM][2];
  Affine8 af;                                              // PRE only
  // PRE: the lane's 8 k-values of chunk c of K-step kt are k = kt * 32 + (2 c + lh) * 8 + e: `tk` = (kt * 32 + c * 16) * 4
  const unsigned t_sc0 = lds0 + (unsigned)(NS * STAGE * 4 + lh * 32);
  auto read_chunk = [&](Ops& o, const unsigned (&ab)[TM][2], unsigned so, unsigned boff, unsigned tk) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      ra[i][0] = lds_rd<0>(ab[i][0] + so);
      ra[i][1] = lds_rd<0>(ab[i][1] + so);
    }
    if constexpr (PRE) {
      af.sc[0] = lds_rd<0>(t_sc0 + tk);
      af.sc[1] = lds_rd<16>(t_sc0 + tk);
      af.sh[0] = lds_rd<0>(t_sc0 + tk + (unsigned)(p.Kp * 4));
      af.sh[1] = lds_rd<16>(t_sc0 + tk + (unsigned)(p.Kp * 4));
    }
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < P; ++q) o.b[j][q] = as_bf(lds_rd<0>(b_base + so + boff + (unsigned)(q * BN * 16 + j * 512)));
  };
  constexpr int NPRE = P == 3 ? 2 : P - 1;                 // products issued before the wait for the next operands
  constexpr int VPM = (split_valu(P, PRE) * TM + (NPROD - NPRE) * TM * TN - 1) / ((NPROD - NPRE) * TM * TN);
  // multiply `cur`; when `fetch`, the reads for `nxt` are already in flight: wait for them after NPRE products and
  // split the A rows under the remaining MFMAs (VPM VALU instructions behind each; about four hide, measured)
  auto multiply = [&](const Ops& cur, Ops& nxt, bool fetch) {
    __builtin_amdgcn_sched_barrier(0);
    mfma_products<TM, TN, 0, NPRE, P>(cur.a, cur.b, acc);
    if (fetch) {
      lgkm_wait();
#pragma unroll
      for (int i = 0; i < TM; ++i) nxt.a[i] = split8<RELU, P, PRE>(ra[i][0], ra[i][1], &af);
      mfma_products<TM, TN, NPRE, NPROD, P>(cur.a, cur.b, acc);
#pragma unroll
      for (int i = 0; i < TM; ++i)                              // keep the split HERE (it would be sunk to its first use)
#pragma unroll
        for (int q = 0; q < P; ++q) asm volatile("" : "+v"(nxt.a[i].p[q]));
#pragma unroll
      for (int u = 0; u < (NPROD - NPRE) * TM * TN; ++u) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // one MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, VPM, 0);    // VPM VALU
      }
    } else {
      mfma_products<TM, TN, NPRE, NPROD, P>(cur.a, cur.b, acc);
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  // chunk (0, 0)
  read_chunk(o0, a_base[0], 0u, 0u, 0u);
  lgkm_wait();
#pragma unroll
  for (int i = 0; i < TM; ++i) o0.a[i] = split8<RELU, P, PRE>(ra[i][0], ra[i][1], &af);

  int cur = 0;
  for (int kt = 0; kt < nk - 1; ++kt) {               // the last K-step is peeled: no branch around the MFMA streams
    const unsigned so = (unsigned)(cur * STAGE * 4);
    // first chunk of the K-step: fetch its second one
    read_chunk(o1, a_base[1], so, (unsigned)(2 * P * BN * 16), (unsigned)((kt * BK + 16) * 4));
    multiply(o0, o1, true);
    // second chunk: open K-step kt+1
    const int nst = cur + 1 == NS ? 0 : cur + 1;
    wait_groups(NS == 3 && kt + 2 < nk ? 1 : 0);
    __syncthreads();
    if (kt + NS < nk) issue(kt + NS, cur);            // stage of K-step kt: every wave has read both of its chunks
    read_chunk(o0, a_base[0], (unsigned)(nst * STAGE * 4), 0u, (unsigned)((kt + 1) * BK * 4));
    multiply(o1, o0, true);
    cur = nst;
  }
  if constexpr (!D2S) pre.template issue<WM, WN>(p, m0, n0, M, epi_vec);   // (D2S reads its residual at the output resolution)
  read_chunk(o1, a_base[1], (unsigned)(cur * STAGE * 4), (unsigned)(2 * P * BN * 16), (unsigned)(((nk - 1) * BK + 16) * 4));
  multiply(o0, o1, true);
  multiply(o1, o0, false);
  }

  if constexpr (D2S) d2s_epilogue<WM, WN, TM, TN>(p, acc, smem, m0, n0, M, epi_vec, cb);
  else conv_epilogue<WM, WN, TM, TN, UP2, true>(p, acc, smem, m0, n0, M, epi_vec, pre);
