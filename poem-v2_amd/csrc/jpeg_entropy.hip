// Huffman decoding of baseline JPEG scans on the device (include/poem_hip.h "baseline JPEG, Huffman decoding on the device").
// The decode step, its bit reader and its checks are csrc/jpeg_entropy.h, shared with the plain-loop host driver of csrc/jpeg.cpp
// (poem_jpeg_entropy_parallel_host): these kernels are that driver with its loops over subsequences spread over the lanes of a
// workgroup.
//
//   jpeg_entropy_kernel   ONE WORKGROUP PER IMAGE, lanes striding over the image's subsequences.  The image's Huffman tables (at
//                         most 6 x 1424 B) and the zig-zag table are staged in LDS; entries, exits, block counts and flags of the
//                         subsequences live in the workspace (62 B each; L2-resident), the one decode
//                         context of the workgroup in LDS (per-lane copies would sit in scratch memory).
//                         Phases, separated by workgroup barriers only:
//                           1. fixed point: every lane whose entry changed decodes its subsequence again, storing nothing, then hands
//                              its exit state to the next lane; until no entry changes (at most as many rounds as subsequences);
//                           2. prefix sum of the block counts (a chunk per lane, the chunk sums scanned by lane 0);
//                           3. write pass: every lane decodes once more from its true entry and stores de-zigzagged coefficients
//                              (DC differences in element 0), each store bounded by the image's own block range;
//                           4. the end of the scan (jpeg_finish, lane 0): block count, EOI grammar, the serial tail where one is due;
//                           5. DC pass: differences -> predictions per component in MCU order, restarting with the restart
//                              intervals, 64-bit sums, a chunk of MCUs per lane and the carries scanned by lane 0.
//                         No workgroup ever waits for another; a workgroup's global stores are read back by its own lanes only behind
//                         a __syncthreads().
//   jpeg_l1_kernel        the range guard: 8 lanes per block sum |coef| * quant (16-byte loads as in jpeg_idct_kernel) and mark the
//                         image RANGE where a block exceeds POEM_JPEG_L1_MAX.
// The per-symbol dependent chain (peek, LDS look-up, shift) is the cost; the streams are read byte by byte through the caches.
#include <hip/hip_runtime.h>
#include "../../include/poem_hip.h"
#include "jpeg.h"
#include "jpeg_entropy.h"

namespace {

constexpr int kMaxLanes = 1024;

__device__ const unsigned char kZigzagDev[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Workspace {
  int* rounds;                   // [n]
  JpegSubState *entry, *exit_, *where;
  int *blocks, *base, *ev;
  unsigned char *cur, *next;
};

__host__ __device__ inline size_t pad16(size_t v) { return (v + 15) & ~(size_t)15; }

__host__ __device__ inline Workspace carve(void* ws, int n, long long subs) {
  Workspace w;
  char* p = (char*)ws;
  w.rounds = (int*)p; p += pad16((size_t)n * 4);
  w.entry = (JpegSubState*)p; p += (size_t)subs * sizeof(JpegSubState);
  w.exit_ = (JpegSubState*)p; p += (size_t)subs * sizeof(JpegSubState);
  w.where = (JpegSubState*)p; p += (size_t)subs * sizeof(JpegSubState);
  w.blocks = (int*)p; p += (size_t)subs * 4;
  w.base = (int*)p; p += (size_t)subs * 4;
  w.ev = (int*)p; p += (size_t)subs * 4;
  w.cur = (unsigned char*)p; p += (size_t)subs;
  w.next = (unsigned char*)p;
  return w;
}

__device__ inline void refuse(poem_jpeg_desc_t* descs, int* status, int i, int code) {
  status[i] = code;
  descs[i].status = code;
}

__global__ __launch_bounds__(kMaxLanes) void jpeg_entropy_kernel(poem_jpeg_desc_t* __restrict__ descs, const poem_jpeg_scan_t* __restrict__ scans,
                                                                 const poem_jpeg_huff_t* __restrict__ tables, long long table_count,
                                                                 const unsigned char* __restrict__ packed, long long packed_bytes, int n,
                                                                 int S, long long total_subs, int16_t* __restrict__ coef,
                                                                 long long coef_bytes, int* __restrict__ status, void* ws_raw) {
  __shared__ __attribute__((aligned(16))) poem_jpeg_huff_t tabs[6];
  __shared__ unsigned char zz[64];
  __shared__ long long dsum[3 * kMaxLanes];
  __shared__ int psum[kMaxLanes];
  __shared__ unsigned char dreset[kMaxLanes];
  __shared__ int sh_event_sub, sh_err, sh_status;

  const int img = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const Workspace w = carve(ws_raw, n, total_subs);
  if (tid == 0) w.rounds[img] = 0;
  const poem_jpeg_desc_t& d = descs[img];
  const poem_jpeg_scan_t s = scans[img];
  if (d.status != 0) {                                            // refused at the header stage: the status stands
    if (tid == 0) status[img] = d.status;
    return;
  }
  // nothing of the records is trusted: whatever does not hang together refuses the image (uniformly over the workgroup)
  bool ok = jpeg_scan_desc_ok(d) && d.coef_offset <= coef_bytes && jpeg_desc_blocks(d) * 128 <= coef_bytes - d.coef_offset;
  ok = ok && s.byte_offset >= 0 && s.byte_count >= 0 && (s.byte_offset & 15) == 0 && s.byte_offset <= packed_bytes &&
       s.byte_count <= packed_bytes - s.byte_offset && ((s.byte_count + 15) & ~15ll) <= packed_bytes - s.byte_offset;
  ok = ok && s.sub_count >= 0 && s.sub_count <= (1 << 30) && (long long)s.sub_count == (s.byte_count + S - 1) / S && s.sub_base >= 0 && s.sub_base <= total_subs &&
       s.sub_count <= total_subs - s.sub_base;
  ok = ok && s.table_count >= 1 && s.table_count <= 6 && s.table_base >= 0 && s.table_base <= table_count &&
       s.table_count <= table_count - s.table_base && s.restart >= 0 && s.restart <= 65535;
  for (int k = 0; k < 3; ++k) ok = ok && s.dc_sel[k] < s.table_count && s.ac_sel[k] < s.table_count;
  if (!ok) {
    if (tid == 0) refuse(descs, status, img, JPEG_EV_MALFORMED);
    return;
  }
  {
    const int* src = reinterpret_cast<const int*>(tables + s.table_base);
    int* dst = reinterpret_cast<int*>(tabs);
    const int words = s.table_count * (int)(sizeof(poem_jpeg_huff_t) / 4);
    for (int k = tid; k < words; k += T) dst[k] = src[k];
    if (tid < 64) zz[tid] = kZigzagDev[tid];
    if (tid == 0) { sh_event_sub = 0x7fffffff; sh_err = 0; sh_status = 0; }
  }
  // ONE context per workgroup, in LDS: every lane reads the same fields (broadcast reads), and per-lane copies would live in
  // scratch memory (the component index into its arrays is dynamic), a global-memory round trip per symbol
  __shared__ JpegScanCtx c;
  if (tid == 0) {
    jpeg_scan_geometry(d, c);
    c.data = packed + s.byte_offset; c.n = s.byte_count; c.zigzag = zz; c.restart = s.restart;
    for (int k = 0; k < 3; ++k) { c.dc[k] = &tabs[s.dc_sel[k]]; c.ac[k] = &tabs[s.ac_sel[k]]; }
  }
  int16_t* const own = coef + d.coef_offset / 2;
  const int nsub = s.sub_count;
  JpegSubState* entry = w.entry + s.sub_base;
  JpegSubState* exit_ = w.exit_ + s.sub_base;
  JpegSubState* where = w.where + s.sub_base;
  int* blocks = w.blocks + s.sub_base;
  int* base = w.base + s.sub_base;
  int* ev = w.ev + s.sub_base;
  unsigned char* cur = w.cur + s.sub_base;
  unsigned char* next = w.next + s.sub_base;
  for (int i = tid; i < nsub; i += T) {
    entry[i] = JpegSubState{(long long)i * S * 8, 0, 0};
    cur[i] = 1; next[i] = 0;
  }
  __syncthreads();

  // 1. the fixed point
  int rounds = 0;
  JpegNoSink none;
  for (bool any = nsub > 0; any && rounds < nsub;) {
    ++rounds;
    for (int i = tid; i < nsub; i += T) {
      if (!cur[i]) continue;
      JpegSubState st = entry[i];
      int done = 0, e = JPEG_EV_RUN;
      if (st.bit >= 0) e = jpeg_sub_decode(c, st, (long long)(i + 1) * S * 8, false, done, none);
      if (e != JPEG_EV_RUN) { where[i] = st; st = JpegSubState{(long long)(i + 1) * S * 8, 0, 0}; }   // the next lane keeps its guess
      exit_[i] = st;
      blocks[i] = done; ev[i] = e;
    }
    __syncthreads();
    int changed = 0;
    for (int i = tid; i < nsub; i += T) {
      if (!cur[i]) continue;
      cur[i] = 0;
      if (i + 1 < nsub && !jpeg_state_eq(exit_[i], entry[i + 1])) {
        entry[i + 1] = exit_[i];
        next[i + 1] = 1;
        changed = 1;
      }
    }
    any = __syncthreads_or(changed) != 0;
    unsigned char* t = cur; cur = next; next = t;
  }

  // 2. the first block of every subsequence, and the one event of the converged trace
  const int chunk = (nsub + T - 1) / T;
  {
    int sum = 0;
    for (int i = tid * chunk; i < min(nsub, (tid + 1) * chunk); ++i) {
      sum += blocks[i];
      if (ev[i] != JPEG_EV_RUN) atomicMin(&sh_event_sub, i);       // the FIRST event counts: behind it lanes ran from guesses
    }
    psum[tid] = sum;
  }
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int t = 0; t < T; ++t) {
      const int v = psum[t];
      psum[t] = (int)(run > 0x7fffffff ? 0x7fffffff : run);
      run += v;
    }
  }
  __syncthreads();
  {
    int run = psum[tid];
    for (int i = tid * chunk; i < min(nsub, (tid + 1) * chunk); ++i) {
      base[i] = run;
      const long long nxt = (long long)run + blocks[i];
      run = nxt > 0x7fffffff ? 0x7fffffff : (int)nxt;
    }
  }
  __syncthreads();

  // 3. the write pass, up to the event
  const int last = sh_event_sub < nsub ? sh_event_sub + 1 : nsub;
  for (int i = tid; i < last; i += T) {
    JpegSubState st = entry[i];
    if (st.bit < 0) continue;
    JpegCoefSink sink;
    sink.start(&c, own, base[i]);
    int done = 0;
    jpeg_sub_decode(c, st, (long long)(i + 1) * S * 8, false, done, sink);
    if (sink.err) sh_err = sink.err;
  }
  __syncthreads();

  // 4. the end of the scan
  if (tid == 0) {
    const int j = sh_event_sub < nsub ? sh_event_sub : -1;
    int st = sh_err;
    const JpegSubState at = j >= 0 ? where[j] : JpegSubState{0, 0, 0};
    const int fin = jpeg_finish(c, j >= 0 ? ev[j] : JPEG_EV_RUN, at, j >= 0 ? (long long)base[j] + blocks[j] : 0, own);
    if (fin) st = fin;
    sh_status = st;
    w.rounds[img] = rounds;
  }
  __syncthreads();
  if (sh_status != 0) {
    if (tid == 0) refuse(descs, status, img, sh_status);
    return;
  }

  // 5. the DC pass
  const long long mchunk = (c.total_mcus + T - 1) / T;
  const long long m0 = min(c.total_mcus, tid * mchunk), m1 = min(c.total_mcus, (tid + 1) * mchunk);
  {
    long long sum[3] = {0, 0, 0};
    bool reset = false;
    JpegCoefSink walk;
    walk.start(&c, own, m0 * c.bpm);
    for (long long mcu = m0; mcu < m1; ++mcu) {
      if (c.restart && mcu && mcu % c.restart == 0) { sum[0] = sum[1] = sum[2] = 0; reset = true; }
      for (int slot = 0; slot < c.bpm; ++slot, walk.next_block()) {
        const int comp = slot < c.hs * c.vs ? 0 : slot - c.hs * c.vs + 1;
        if (walk.blk) sum[comp] += walk.blk[0];
      }
    }
    for (int k = 0; k < 3; ++k) dsum[k * kMaxLanes + tid] = sum[k];
    dreset[tid] = reset;
  }
  __syncthreads();
  if (tid == 0) {
    long long carry[3] = {0, 0, 0};
    for (int t = 0; t < T; ++t)
      for (int k = 0; k < 3; ++k) {
        const long long v = dsum[k * kMaxLanes + t];
        dsum[k * kMaxLanes + t] = carry[k];
        carry[k] = dreset[t] ? v : carry[k] + v;
      }
  }
  __syncthreads();
  {
    long long pred[3] = {dsum[tid], dsum[kMaxLanes + tid], dsum[2 * kMaxLanes + tid]};
    bool bad = false;
    JpegCoefSink walk;
    walk.start(&c, own, m0 * c.bpm);
    for (long long mcu = m0; mcu < m1; ++mcu) {
      if (c.restart && mcu && mcu % c.restart == 0) pred[0] = pred[1] = pred[2] = 0;
      for (int slot = 0; slot < c.bpm; ++slot, walk.next_block()) {
        const int comp = slot < c.hs * c.vs ? 0 : slot - c.hs * c.vs + 1;
        if (!walk.blk) continue;
        pred[comp] += walk.blk[0];
        if (pred[comp] < -32768 || pred[comp] > 32767) bad = true;
        walk.blk[0] = (int16_t)pred[comp];
      }
    }
    if (bad) sh_status = JPEG_EV_MALFORMED;
  }
  __syncthreads();
  if (tid == 0) {
    status[img] = sh_status;
    if (sh_status) descs[img].status = sh_status;
  }
}

// last i in [0, n) with block_base(i) <= idx (as in csrc/jpeg.hip)
__device__ __forceinline__ int find_image(const poem_jpeg_desc_t* descs, int n, long long idx) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].block_base <= idx) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void jpeg_l1_kernel(poem_jpeg_desc_t* __restrict__ descs, const int16_t* __restrict__ coef,
                                                      long long coef_bytes, int n, long long total_blocks, int* __restrict__ status) {
  const int r = threadIdx.x & 7;
  const long long gb = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
  int l1 = 0, img = 0;
  bool live = gb < total_blocks;
  if (live) {
    img = find_image(descs, n, gb);
    const poem_jpeg_desc_t& d = descs[img];
    long long local = gb - d.block_base;
    live = jpeg_desc_ok(d) && local < jpeg_desc_blocks(d) && d.coef_offset <= coef_bytes && (local + 1) * 128 <= coef_bytes - d.coef_offset;
    if (live) {
      const int4 cv = *reinterpret_cast<const int4*>(reinterpret_cast<const char*>(coef) + d.coef_offset + local * 128 + r * 16);
      int comp = 0;
      while (comp + 1 < d.ncomp && local >= (long long)d.blocks_w[comp] * d.blocks_h[comp]) {
        local -= (long long)d.blocks_w[comp] * d.blocks_h[comp];
        ++comp;
      }
      const int4 qv = *reinterpret_cast<const int4*>(&d.quant[comp][r * 8]);
      const int cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {                                // |int16| x uint16 <= 2^31 / 64: eight of them fit an int
        l1 += abs((int)(short)(cw[k] & 0xffff)) * (int)(qw[k] & 0xffff);
        l1 += abs(cw[k] >> 16) * (int)((unsigned)qw[k] >> 16);
      }
    }
  }
  // the 8 lanes of a block: |coef| <= 32768 and quant <= 255 keep the block's sum below 2^30
  l1 += __shfl_xor(l1, 1);
  l1 += __shfl_xor(l1, 2);
  l1 += __shfl_xor(l1, 4);
  if (live && r == 0 && l1 > POEM_JPEG_L1_MAX) {
    status[img] = JPEG_EV_RANGE;
    descs[img].status = JPEG_EV_RANGE;
  }
}

}  // namespace

extern "C" size_t poem_jpeg_entropy_ws_bytes(int n, long long total_subs) {
  if (n <= 0 || total_subs < 0) return 0;
  return pad16((size_t)n * 4) + pad16((size_t)total_subs * (3 * sizeof(JpegSubState) + 3 * 4 + 2)) + 16;
}

extern "C" hipError_t poem_launch_jpeg_entropy(poem_jpeg_desc_t* descs, const poem_jpeg_scan_t* scans, const poem_jpeg_huff_t* tables,
                                               long long table_count, const unsigned char* packed, long long packed_bytes, int n, int subseq,
                                               int wg_threads, long long total_subs, long long total_blocks, int16_t* coef,
                                               long long coef_bytes, int* status, void* workspace, hipStream_t s) {
  hipError_t e = coef_bytes > 0 ? hipMemsetAsync(coef, 0, (size_t)coef_bytes, s) : hipSuccess;
  if (e != hipSuccess) return e;
  jpeg_entropy_kernel<<<dim3((unsigned)n), dim3((unsigned)wg_threads), 0, s>>>(descs, scans, tables, table_count, packed, packed_bytes, n,
                                                                             subseq, total_subs, coef, coef_bytes, status, workspace);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (total_blocks > 0)
    jpeg_l1_kernel<<<dim3((unsigned)((total_blocks + 31) / 32)), dim3(256), 0, s>>>(descs, coef, coef_bytes, n, total_blocks, status);
  return hipGetLastError();
}
