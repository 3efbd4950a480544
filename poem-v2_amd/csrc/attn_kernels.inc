// The exact-fp32 cross-attention kernels of attn.hip, compiled twice from this one text (attn.hip includes it with the names
// below defined): once as xattn_half_item / xattn_kernel / xattn_stream_kernel, and once -- XA_MASKED 1 -- as their MASK twins
// xattn_masked_half_item / xattn_masked_kernel / xattn_stream_masked_kernel for a key count that is not a multiple of 32
// (POEM_MASK_TAIL, attn.hip).  A textual include instead of a template parameter or a shared inline body: the unmasked kernels
// keep their names AND their machine code (a forwarding kernel around a shared body re-schedules the softmax).
//   XA_HALF_ITEM, XA_KERNEL, XA_STREAM_KERNEL   the three names        XA_MASKED   0 | 1

// ---- round 6: the REMAINDER items of a launch as channel-tile halves.  The static map deals a CU pair's n items to its 8 W waves
// round-robin: n = 100 at the headline batch, 24 waves -> four full rounds and a remainder of 4 items, which four of the pair's
// eight SIMDs run as a 13th item while the other four idle (12.5 items per SIMD on average, 13 on the busiest: the kernel's
// 0.96 quantisation; at 64 samples, 25.0 items per SIMD, the same kernel is 0.885 MFMA-busy instead of 0.845).  A remainder of
// r <= 4 items is dealt as 2 r HALF items instead, one per SIMD of the pair: the item's full score contraction and softmax but
// ONE 32-channel tile of P V (48 instead of 64 MFMAs per key tile, the HALF idea of the merged kernel), so the last round is
// 0.75 of an item on every SIMD instead of a whole one on half of them.  Each output element of the partial is the same fma
// chain over the keys whichever wave owns its channel tile, and (m, l) -- functions of the scores only -- are written by the
// tile-0 half: bit-identical partials, same layout.
template <int DH>
__device__ __forceinline__ void XA_HALF_ITEM(const float* __restrict__ q, int ldq, int qbr, const __amdgpu_buffer_rsrc_t krs,
                                                const __amdgpu_buffer_rsrc_t vrs, float4* __restrict__ part_o,
                                                float2* __restrict__ part_ml, int item, int d0, int nqt, int chunks, int heads, int NQ,
                                                int nkt, int C, int tpc, float kc2, float lazy_raw
#if XA_MASKED
                                                , int dead
#endif
                                                ) {
  constexpr int KC = DH / 8, DTF = DH / 32, DT = 1;
  // (the lane id afresh from the hardware -- mbcnt -- instead of the kernel's `lane`: keeping that one alive across the main
  //  item loop for this tail was the 169th register of a kernel that fits three waves per SIMD in 168)
  const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const int r = lane & 31, h = lane >> 5, loff = lane * 16;
  const int qt = item % nqt;
  int t = item / nqt;
  const int ch = t % chunks;
  t /= chunks;
  const int head = t % heads, b = t / heads;
  const int qrow = min(qt * 32 + r, NQ - 1);
  float4 qf[KC];
  {
    const float* qp = q + ((size_t)b * qbr + qrow) * ldq + head * DH + 4 * h;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) qf[kc] = *reinterpret_cast<const float4*>(qp + 8 * kc);
  }
  const int kt0 = ch * tpc;
  const int ktile_bytes = C * 128;
  int koff = __builtin_amdgcn_readfirstlane((b * nkt + kt0) * ktile_bytes + head * KC * 1024);
  int voff = __builtin_amdgcn_readfirstlane((b * nkt + kt0) * ktile_bytes + ((head * DH) / 32 + d0) * 4096);
  float4 kf[KC], vf[DT][4];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc) kf[kc] = frag_load(krs, loff, koff + kc * 1024);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int g = 0; g < 4; ++g) vf[0][g] = frag_load(vrs, loff, voff + g * 1024);
  __builtin_amdgcn_sched_barrier(0);
  f32x16 o[DT];
  o[0] = zero16();
  float m_ref = -INFINITY, nbias = 0.f, l_run = 0.f;
  for (int kt = 0; kt < tpc; ++kt) {
    if ((kt & 3) == 0 && kt) __builtin_amdgcn_s_barrier();      // (as the full items: the block's live waves stay on the same tiles)
    f32x16 s = zero16();
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      s = mfma32(kf[kc].x, qf[kc].x, s);
      s = mfma32(kf[kc].y, qf[kc].y, s);
      s = mfma32(kf[kc].z, qf[kc].z, s);
      s = mfma32(kf[kc].w, qf[kc].w, s);
    }
    __builtin_amdgcn_sched_barrier(0);
    const int adv = (kt + 1 < tpc) ? ktile_bytes : 0;
    koff += adv;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) kf[kc] = frag_load(krs, loff, koff + kc * 1024);
    __builtin_amdgcn_sched_barrier(0);
#if XA_MASKED
    POEM_MASK_TAIL(kt == tpc - 1 && ch == chunks - 1)
#endif
    POEM_SOFTMAX_TILE(DT)
    __builtin_amdgcn_sched_barrier(0);
    voff += adv;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      o[0] = mfma32((&vf[0][i >> 2].x)[i & 3], s[i], o[0]);
      if ((i & 3) == 3) {
        __builtin_amdgcn_sched_barrier(0);
        vf[0][i >> 2] = frag_load(vrs, loff, voff + (i >> 2) * 1024);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  l_run = half_sum(l_run);
  float4* po = part_o + (size_t)item * (DTF * 4) * 64 + lane;
#pragma unroll
  for (int g = 0; g < 4; ++g) nt_store4(po + (d0 * 4 + g) * 64, make_float4(o[0][4 * g], o[0][4 * g + 1], o[0][4 * g + 2], o[0][4 * g + 3]));
  if (h == 0 && d0 == 0) part_ml[(size_t)item * 32 + r] = make_float2(m_ref, l_run);
  __builtin_amdgcn_s_waitcnt(0x0F70);
}

// MERGE (round 3; four key chunks, the head path's shape): the four chunks of a query tile run on four waves of ONE block at
// the same time -- wave w = (group w / 4, chunk w % 4), a block's W groups take consecutive query tiles -- and the block
// merges their partials through LDS (attn_combine_kernel's arithmetic, chunk order) and writes the normalised context rows:
// the partials (4 x 26 MB written per launch at the headline batch and read back by the consumer) never reach HBM.  The waves
// of a group read different K/V chunks, the W waves with the same chunk the same one (the tile barrier keeps them together).
// HALF (MERGE only, round 4): an item is one 32-channel tile of a query tile's output instead of all DH / 32 of them -- twice the
// items, each with the full score contraction and softmax but half the P V products (48 instead of 64 MFMAs per key tile).  More
// MFMAs in all, so it only pays where the launch is one under-filled round anyway: a single sample (100 query-tile items on 256
// CUs -> 200).  Every output element is the same fma chain as without it.
template <int DH, int W, bool MERGE = false, bool HALF = false>
__global__ __launch_bounds__(256 * W, W) void XA_KERNEL(const float* __restrict__ q, int ldq, int qbr,
                                                           const float4* __restrict__ kimg,
                                                           const float4* __restrict__ vimg,
                                                           float4* __restrict__ part_o, float2* __restrict__ part_ml,
                                                           int B, int NQ, int NK, int C, int heads, int tpc, float kc2,
                                                           float lazy_raw, int map, int prio_rot, float* __restrict__ ctx) {
  const bool split_tail = (map & 16) != 0;      // (bit 4 of `map`: the remainder items as halves)
#if XA_MASKED
  const int dead = (map >> 8) & 31;             // bits 8..12 of `map`: columns of the last key tile behind the last key
#endif
  map &= 15;
  constexpr int KC = DH / 8;               // K fragments (float4) per key tile
  constexpr int DTF = (DH + 31) / 32;      // 32-channel tiles of the output
  constexpr int DT = HALF ? 1 : DTF;       // ... of an item
  static_assert(!HALF || MERGE, "channel-tile items exist in the merged form only");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int nqt = (NQ + 31) / 32, nkt = NK / 32, chunks = nkt / tpc;
  const int items = MERGE ? B * heads * nqt * (HALF ? DTF : 1) : B * heads * chunks * nqt;      // MERGE: one item = a query tile, all four chunks
  extern __shared__ __attribute__((aligned(16))) float xa_lds[];            // MERGE: 4W x (DT*4 x 64 float4 | 32 float2)
  // logical block id: blocks of one XCD (blockIdx % 8) take neighbouring item ranges -> one L2 serves a K/V chunk
  const int nb = gridDim.x;
  const int lb = (nb % 8 == 0) ? (int)(blockIdx.x % 8) * (nb / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  // map 1: a CU owns a contiguous item range and deals it round-robin to all its waves (wave w sits on SIMD w % 4, so
  //        the SIMDs stay balanced to within one item) -- every wave of the CU streams the same K/V chunk at the same
  //        time: one HBM/L2 fetch serves them all.
  // map 0: each SIMD owns a contiguous range, dealt to its W waves.
  // map 2: TWO neighbouring blocks of an XCD (logical ids 2k, 2k + 1) share a contiguous item range and deal it round-robin to
  //        their 8 W waves: the 25 query tiles of a (sample, head, key chunk) group then meet its K / V chunk in one sweep of two
  //        CUs instead of 2.1 sweeps of one (each sweep beyond the first re-fetches the chunk: 16 MB of chunks per XCD do not
  //        stay in its 4 MB L2).
  const bool pair = !MERGE && map == 2 && nb % 16 == 0;
  const int sg = pair ? (lb >> 1) : ((map || MERGE) ? lb : lb * 4 + (wv & 3)), ng = pair ? (nb >> 1) : ((map || MERGE) ? nb : nb * 4);
  const int ibase = items / ng, irem = items % ng;
  const int lo = ibase * sg + min(sg, irem), hi = lo + ibase + (sg < irem ? 1 : 0);
  const int first = MERGE ? (wv >> 2) : (pair ? 2 * wv + (lb & 1) : (map ? wv : (wv >> 2)));      // (pair: the two blocks' waves alternate)
  const int stride = MERGE ? W : (pair ? 8 * W : (map ? 4 * W : W));
  const __amdgpu_buffer_rsrc_t krs = frag_rsrc(kimg, 0xffffffffu), vrs = frag_rsrc(vimg, 0xffffffffu);
  const int loff = lane * 16;
  const bool sync_tiles = MERGE || (map != 0 && prio_rot != 3);      // (prio_rot == 3: lab switch to turn the tile barrier off)
#ifdef POEM_LAB
  const long long dbg_c0 = clock64(), dbg_w0 = wall_clock64();
  int dbg_items = 0;
#endif
#ifdef POEM_XA_STAMPS
  const bool dbg_on = blockIdx.x == 5 && wv == 0;
  long long dbg_ph[4] = {0, 0, 0, 0}, dbg_last = 0;
#endif

  // (pair map, head dim 64: a remainder of <= 4 items behind the full rounds runs as halves -- xattn_half_item above)
  // (wave-uniform values the compiler cannot prove uniform -- they derive from threadIdx -- pinned to scalar registers: the
  //  kernel sits at its 168-register budget for three waves per SIMD)
  int hi_full = hi;
  if constexpr (!MERGE && DH == 64) {
    const int rem = (hi - lo) % stride;
    if (pair && split_tail && rem > 0 && 2 * rem <= 8 && W == 3) hi_full = hi - rem;
    hi_full = __builtin_amdgcn_readfirstlane(hi_full);
  }
  const int tail_items = __builtin_amdgcn_readfirstlane(hi - hi_full), tail_first = __builtin_amdgcn_readfirstlane(first);
  for (int item = lo + first; item < hi_full; item += stride) {
#ifdef POEM_LAB
    ++dbg_items;
#endif
    const int d0 = HALF ? item % DTF : 0;      // first output channel tile of this item
    const int qt = (HALF ? item / DTF : item) % nqt;
    int t = (HALF ? item / DTF : item) / nqt;
    const int ch = MERGE ? (wv & 3) : t % chunks;
    if (!MERGE) t /= chunks;
    const int head = t % heads, b = t / heads;
    const int qrow = min(qt * 32 + r, NQ - 1);

    // Q fragment: lane (query r, half h) holds Q[r][8kc + 4h + t]
    float4 qf[KC];
    {
      const float* qp = q + ((size_t)b * qbr + qrow) * ldq + head * DH + 4 * h;
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) qf[kc] = *reinterpret_cast<const float4*>(qp + 8 * kc);
    }
    // scalar byte offsets of this item's first key tile in the two images
    const int kt0 = ch * tpc;
    const int ktile_bytes = C * 128;                                        // 32 keys x C floats, both images
    int koff = __builtin_amdgcn_readfirstlane((b * nkt + kt0) * ktile_bytes + head * KC * 1024);
    int voff = __builtin_amdgcn_readfirstlane((b * nkt + kt0) * ktile_bytes + ((head * DH) / 32) * 4096);

    float4 kf[KC], vf[DT][4];
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) kf[kc] = frag_load(krs, loff, koff + kc * 1024);
    __builtin_amdgcn_sched_barrier(0);   // issue order Q, K, V as in the loop: the loop header then waits for K only
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) vf[d][g] = frag_load(vrs, loff, voff + ((d0 + d) * 4 + g) * 1024);
    __builtin_amdgcn_sched_barrier(0);

    f32x16 o[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) o[d] = zero16();
    float m_ref = -INFINITY, nbias = 0.f, l_run = 0.f;

    for (int kt = 0; kt < tpc; ++kt) {
      XA_STAMP(0);
      // A block barrier every 4 key tiles keeps all waves of the CU (they stream the same K/V chunk, map 1) within 4 tiles
      // of each other, so one fetch from HBM / Infinity Cache serves all 12 of them through L2: 3.4 -> 1.0 GB fetched per
      // launch, -3.6 % kernel time, and less cache pollution for the kernels that follow.  Left alone the waves drift by
      // whole items (the arbiter serves the oldest wave of a SIMD first).  Waves that ran out of items have exited; a
      // terminated wave no longer counts at the barrier.
      if (sync_tiles && (kt & 3) == 0 && kt) __builtin_amdgcn_s_barrier();
#ifdef POEM_LAB   // experiment kept for the lab build only (does not pay; DESIGN.md)
      if (W > 1 && prio_rot == 1) {
        const int pr = (kt + (wv >> 2)) % W;
        if (pr == 0) __builtin_amdgcn_s_setprio(0);
        else if (pr == 1) __builtin_amdgcn_s_setprio(1);
        else if (pr == 2) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(3);
      }
#endif
      // ---- S^T = K . Q^T (raw scores)
      f32x16 s = zero16();
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        s = mfma32(kf[kc].x, qf[kc].x, s);
        s = mfma32(kf[kc].y, qf[kc].y, s);
        s = mfma32(kf[kc].z, qf[kc].z, s);
        s = mfma32(kf[kc].w, qf[kc].w, s);
      }
      __builtin_amdgcn_sched_barrier(0);
      // next tile's K fragments into the registers the MFMAs above have just read (clamped: the last prefetch of an
      // item re-reads its own last tile)
      const int adv = (kt + 1 < tpc) ? ktile_bytes : 0;
      koff += adv;
#ifndef POEM_XA_NOLOADS
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) kf[kc] = frag_load(krs, loff, koff + kc * 1024);
#endif
      __builtin_amdgcn_sched_barrier(0);

      XA_STAMP(1);
#if XA_MASKED
      POEM_MASK_TAIL(kt == tpc - 1 && ch == chunks - 1)
#endif
      // ---- softmax numerators, lazy stabiliser
      POEM_SOFTMAX_TILE(DT)
      __builtin_amdgcn_sched_barrier(0);
      XA_STAMP(2);

      // ---- O^T += V^T . P^T; the V fragments of register group g are re-requested (next tile) as soon as the four
      //      k-steps that read them have been issued
      voff += adv;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
#pragma unroll
        for (int d = 0; d < DT; ++d) o[d] = mfma32((&vf[d][i >> 2].x)[i & 3], s[i], o[d]);
        if ((i & 3) == 3) {
          __builtin_amdgcn_sched_barrier(0);
#ifndef POEM_XA_NOLOADS
#pragma unroll
          for (int d = 0; d < DT; ++d) vf[d][i >> 2] = frag_load(vrs, loff, voff + ((d0 + d) * 4 + (i >> 2)) * 1024);
#endif
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      XA_STAMP(3);
    }

    l_run = half_sum(l_run);
    if constexpr (MERGE) {
      // ---- the four chunk partials of this wave's group meet in LDS (fragment order, as the HBM partials)
      constexpr int WSTRIDE = DT * 4 * 64 * 4 + 64;          // floats per wave: O image | (m, l) of its 32 rows
      float* mine = xa_lds + wv * WSTRIDE;
#pragma unroll
      for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          reinterpret_cast<float4*>(mine)[(d * 4 + g) * 64 + lane] = make_float4(o[d][4 * g], o[d][4 * g + 1], o[d][4 * g + 2], o[d][4 * g + 3]);
      if (h == 0) reinterpret_cast<float2*>(mine + DT * 4 * 64 * 4)[r] = make_float2(m_ref, l_run);
      __syncthreads();                        // every live wave is at the end of an item (all items have tpc tiles)
      // ---- ctx[b, q, head*DH + c] = sum_s w_s O_s[c] / sum_s w_s l_s (attn_combine_kernel, chunk order); chunk-wave c of the
      // group takes float4 groups c, c + 4, ... of the DT * 4
      const float* grp = xa_lds + (wv & ~3) * WSTRIDE;
      float w4[4], M = -INFINITY, den = 0.f;
#pragma unroll
      for (int sx = 0; sx < 4; ++sx) {
        w4[sx] = reinterpret_cast<const float2*>(grp + sx * WSTRIDE + DT * 4 * 64 * 4)[r].x;
        M = fmaxf(M, w4[sx]);
      }
#pragma unroll
      for (int sx = 0; sx < 4; ++sx) {
        const float lx = reinterpret_cast<const float2*>(grp + sx * WSTRIDE + DT * 4 * 64 * 4)[r].y;
        w4[sx] = (w4[sx] == M) ? 1.0f : __builtin_amdgcn_exp2f((w4[sx] - M) * kc2);
        den = fmaf(w4[sx], lx, den);
      }
      if (qt * 32 + r < NQ) {
        float* out = ctx + ((size_t)b * NQ + qt * 32 + r) * C + head * DH;
#pragma unroll
        for (int k = (wv & 3); k < DT * 4; k += 4) {
          float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int sx = 0; sx < 4; ++sx) {
            const float4 pp = reinterpret_cast<const float4*>(grp + sx * WSTRIDE)[k * 64 + lane];
            acc.x = fmaf(w4[sx], pp.x, acc.x); acc.y = fmaf(w4[sx], pp.y, acc.y);
            acc.z = fmaf(w4[sx], pp.z, acc.z); acc.w = fmaf(w4[sx], pp.w, acc.w);
          }
          const int d = d0 + (k >> 2), g = k & 3;
          *reinterpret_cast<float4*>(out + 32 * d + 8 * g + 4 * h) = make_float4(acc.x / den, acc.y / den, acc.z / den, acc.w / den);
        }
      }
      // (the next item's tile barriers -- tpc >= 8, checked at launch -- order these reads before its LDS writes)
    } else {
      // partial (O, m, l): fragment order, one coalesced 1 KiB store per (channel tile, register group)
      float4* po = part_o + (size_t)item * (DT * 4) * 64 + lane;
#pragma unroll
      for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          nt_store4(po + (d * 4 + g) * 64, make_float4(o[d][4 * g], o[d][4 * g + 1], o[d][4 * g + 2], o[d][4 * g + 3]));
      if (h == 0) part_ml[(size_t)item * 32 + r] = make_float2(m_ref, l_run);
    }
    // drain the stores here: with stores possibly pending at the key loop's header hipcc cannot count on in-order
    // returns and waits for vmcnt(0) on every iteration, i.e. for the V prefetch it has just issued
    __builtin_amdgcn_s_waitcnt(0x0F70);
  }
  if constexpr (!MERGE && DH == 64) {
    // halves of the remainder: pair-wave index `first` (even: first block of the pair, odd: second) -> SIMD first % 8 of the pair
    if (tail_first < 2 * tail_items)
      XA_HALF_ITEM<DH>(q, ldq, qbr, krs, vrs, part_o, part_ml, hi_full + (tail_first >> 1), tail_first & 1, nqt, chunks, heads, NQ, nkt, C,
                          tpc, kc2, lazy_raw
#if XA_MASKED
                          , dead
#endif
                          );
  }
#ifdef POEM_LAB
  if (lane == 0) {
    long long* d = &xattn_dbg[((size_t)blockIdx.x * 4 * W + wv) % 4096 * 4];
    d[0] = clock64() - dbg_c0; d[1] = wall_clock64() - dbg_w0; d[2] = dbg_items; d[3] = blockIdx.x;
  }
#endif
#ifdef POEM_XA_STAMPS
  if (dbg_on && lane == 0) for (int i = 0; i < 4; ++i) xattn_ph[i] = dbg_ph[i];
#endif
}

// Head dims 128 and 256 (POEM-large / -huge): the K and V fragments of a key tile no longer fit the register file next
// to Q and O, so they stream through a two-slot ring of 8 fragments (32 registers each): a tile is a fixed sequence of
// NG = DH/64 + DH/64 operand groups -- K channel groups of 64, then V channel-tile pairs -- and while the 32 MFMAs of
// group n issue, group n+1 (the next tile's first K group after the last V pair) is in flight into the other slot.
// NG is even, so the slot of every group is a compile-time constant.  Same items, partials and combine as above.
template <int DH, int W>
__global__ __launch_bounds__(256 * W, W) void XA_STREAM_KERNEL(const float* __restrict__ q, int ldq, int qbr,
                                                                  const float4* __restrict__ kimg,
                                                                  const float4* __restrict__ vimg,
                                                                  float4* __restrict__ part_o,
                                                                  float2* __restrict__ part_ml, int B, int NQ, int NK,
                                                                  int C, int heads, int tpc, float kc2, float lazy_raw,
                                                                  int map) {
  constexpr int KC = DH / 8, DT = DH / 32, NGK = KC / 8, NGV = DT / 2;
  static_assert(NGK == NGV && NGK >= 1, "head dim must be a multiple of 64");
#if XA_MASKED
  const int dead = (map >> 8) & 31;             // bits 8..12 of `map`, as xattn_kernel
  map &= 15;
#endif
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int nqt = (NQ + 31) / 32, nkt = NK / 32, chunks = nkt / tpc;
  const int items = B * heads * chunks * nqt;
  const int nb = gridDim.x;
  const int lb = (nb % 8 == 0) ? (int)(blockIdx.x % 8) * (nb / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int sg = map ? lb : lb * 4 + (wv & 3), ng = map ? nb : nb * 4;
  const int ibase = items / ng, irem = items % ng;
  const int lo = ibase * sg + min(sg, irem), hi = lo + ibase + (sg < irem ? 1 : 0);
  const int first = map ? wv : (wv >> 2), stride = map ? 4 * W : W;
  const __amdgpu_buffer_rsrc_t krs = frag_rsrc(kimg, 0xffffffffu), vrs = frag_rsrc(vimg, 0xffffffffu);
  const int loff = lane * 16;

  for (int item = lo + first; item < hi; item += stride) {
    const int qt = item % nqt;
    int t = item / nqt;
    const int ch = t % chunks;
    t /= chunks;
    const int head = t % heads, b = t / heads;
    const int qrow = min(qt * 32 + r, NQ - 1);
    // The query fragment (KC float4 per lane: 128 registers at head dim 256): in registers for head dim 64; in LDS for the
    // wide heads (a wave's own KC KB, fragment order, conflict-free ds_read_b128 right in front of the MFMAs that use it) --
    // the registers it frees are what the four-group ring below is made of.
    constexpr bool QLDS = NGK >= 2;
    extern __shared__ __attribute__((aligned(16))) float4 xs_q[];      // QLDS: (waves of the block) x KC x 64
    float4* qs = xs_q + (size_t)wv * KC * 64 + lane;
    float4 qf[QLDS ? 1 : KC];
    {
      const float* qp = q + ((size_t)b * qbr + qrow) * ldq + head * DH + 4 * h;
      if constexpr (QLDS) {
        constexpr int QB = 8;
#pragma unroll
        for (int k0 = 0; k0 < KC; k0 += QB) {
          float4 t[QB];
#pragma unroll
          for (int u = 0; u < QB; ++u) t[u] = *reinterpret_cast<const float4*>(qp + 8 * (k0 + u));
#pragma unroll
          for (int u = 0; u < QB; ++u) qs[(k0 + u) * 64] = t[u];
        }
      } else {
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) qf[kc] = *reinterpret_cast<const float4*>(qp + 8 * kc);
      }
    }
    const int kt0 = ch * tpc;
    const int ktile_bytes = C * 128;
    int koff = __builtin_amdgcn_readfirstlane((b * nkt + kt0) * ktile_bytes + head * KC * 1024);
    int voff = __builtin_amdgcn_readfirstlane((b * nkt + kt0) * ktile_bytes + ((head * DH) / 32) * 4096);
    f32x16 o[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) o[d] = zero16();
    float m_ref = -INFINITY, nbias = 0.f, l_run = 0.f;
    if constexpr (NGK >= 2) {
      // Head dims 128 / 256 (round 4): ONE wave per SIMD (the query fragment and the output tiles alone are 192 / 256 registers),
      // so nothing hides a load but the wave's own distance to it -- and one 8 KB group ahead is 32 MFMAs = 0.85 us, less than
      // an L2 / MALL round trip under load.  Ring of FOUR groups, three in flight: the
      // 2 NGK groups of a tile (K groups, then V pairs) are 4 or 8, so every group's slot is a compile-time constant.
      float4 ring[4][8];
      // group n of the current tile: K group n | V pair n - NGK | the NEXT tile's K group n - 2 NGK | its V pair n - 3 NGK
#define XS_LOAD(N, ADV)                                                                                        \
      _Pragma("unroll") for (int e = 0; e < 8; ++e)                                                            \
        ring[(N) & 3][e] = (N) < NGK ? frag_load(krs, loff, koff + ((N) * 8 + e) * 1024)                       \
                         : (N) < 2 * NGK ? frag_load(vrs, loff, voff + (((N) - NGK) * 8 + e) * 1024)           \
                         : (N) < 3 * NGK ? frag_load(krs, loff, koff + (ADV) + (((N) - 2 * NGK) * 8 + e) * 1024) \
                                         : frag_load(vrs, loff, voff + (ADV) + (((N) - 3 * NGK) * 8 + e) * 1024);
      XS_LOAD(0, 0) XS_LOAD(1, 0) XS_LOAD(2, 0)
      __builtin_amdgcn_sched_barrier(0);
      for (int kt = 0; kt < tpc; ++kt) {
        if (map && (kt & 3) == 0 && kt) __builtin_amdgcn_s_barrier();   // keep the CU's waves on the same K/V tiles (see xattn_kernel)
        const int adv = (kt + 1 < tpc) ? ktile_bytes : 0;
        f32x16 s = zero16();
#pragma unroll
        for (int g = 0; g < NGK; ++g) {
          XS_LOAD(g + 3, adv)
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float4 a = ring[g & 3][e];
            const float4 bq = qs[(g * 8 + e) * 64];
            s = mfma32(a.x, bq.x, s);
            s = mfma32(a.y, bq.y, s);
            s = mfma32(a.z, bq.z, s);
            s = mfma32(a.w, bq.w, s);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
#if XA_MASKED
        POEM_MASK_TAIL(kt == tpc - 1 && ch == chunks - 1)
#endif
        POEM_SOFTMAX_TILE(DT)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int v = 0; v < NGV; ++v) {
          XS_LOAD(NGK + v + 3, adv)
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 16; ++i) {
#pragma unroll
            for (int dd = 0; dd < 2; ++dd)
              o[2 * v + dd] = mfma32((&ring[(NGK + v) & 3][dd * 4 + (i >> 2)].x)[i & 3], s[i], o[2 * v + dd]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        koff += adv;
        voff += adv;
      }
#undef XS_LOAD
    } else {
    float4 ring[2][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) ring[0][e] = frag_load(krs, loff, koff + e * 1024);
    __builtin_amdgcn_sched_barrier(0);
    for (int kt = 0; kt < tpc; ++kt) {
      if (map && (kt & 3) == 0 && kt) __builtin_amdgcn_s_barrier();   // keep the CU's waves on the same K/V tiles (see xattn_kernel)
      const int adv = (kt + 1 < tpc) ? ktile_bytes : 0;
      f32x16 s = zero16();
#pragma unroll
      for (int g = 0; g < NGK; ++g) {
        // next group: K group g+1 of this tile, or V pair 0 behind the last K group
#pragma unroll
        for (int e = 0; e < 8; ++e)
          ring[(g + 1) & 1][e] = (g + 1 < NGK) ? frag_load(krs, loff, koff + ((g + 1) * 8 + e) * 1024)
                                               : frag_load(vrs, loff, voff + e * 1024);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float4 a = ring[g & 1][e];
          const float4 bq = qf[g * 8 + e];
          s = mfma32(a.x, bq.x, s);
          s = mfma32(a.y, bq.y, s);
          s = mfma32(a.z, bq.z, s);
          s = mfma32(a.w, bq.w, s);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#if XA_MASKED
      POEM_MASK_TAIL(kt == tpc - 1 && ch == chunks - 1)
#endif
      POEM_SOFTMAX_TILE(DT)
      __builtin_amdgcn_sched_barrier(0);
      koff += adv;
#pragma unroll
      for (int v = 0; v < NGV; ++v) {
        // next group: V pair v+1 of this tile, or the next tile's K group 0 behind the last pair
#pragma unroll
        for (int e = 0; e < 8; ++e)
          ring[(NGK + v + 1) & 1][e] = (v + 1 < NGV) ? frag_load(vrs, loff, voff + ((v + 1) * 8 + e) * 1024)
                                                     : frag_load(krs, loff, koff + e * 1024);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
#pragma unroll
          for (int dd = 0; dd < 2; ++dd)
            o[2 * v + dd] = mfma32((&ring[(NGK + v) & 1][dd * 4 + (i >> 2)].x)[i & 3], s[i], o[2 * v + dd]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      voff += adv;
    }
    }
    l_run = half_sum(l_run);
    float4* po = part_o + (size_t)item * (DT * 4) * 64 + lane;
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        nt_store4(po + (d * 4 + g) * 64, make_float4(o[d][4 * g], o[d][4 * g + 1], o[d][4 * g + 2], o[d][4 * g + 3]));
    if (h == 0) part_ml[(size_t)item * 32 + r] = make_float2(m_ref, l_run);
    __builtin_amdgcn_s_waitcnt(0x0F70);   // see xattn_kernel
  }
}

