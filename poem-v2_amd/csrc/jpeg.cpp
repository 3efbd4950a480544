// Host half of the device JPEG route (include/poem_hip.h "baseline JPEG"): marker parser, Huffman decoder and the plain-loop
// reconstruction over csrc/jpeg.h.  No HIP in here: the file also builds alone (tools/jpeg_hostcheck.cpp).
// Everything a stream says is distrusted: every read goes through Reader (checked against the stream's length), every
// coefficient write through the image's own range, and anything unexpected REFUSES the image -- the caller then uses PIL.
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>
#include <vector>
#include "../../include/poem_hip.h"
#include "jpeg.h"
#include "jpeg_entropy.h"

namespace {

enum { TAKEN = 0, UNSUPPORTED = 1, MALFORMED = 2, RANGE = 3 };

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
  bool defined = false;
  uint16_t look[512];          // 9-bit prefix -> (length << 8) | symbol, 0 = longer than 9 bits (or no such code)
  int32_t maxcode[18];         // largest code of each length (-1: none), [17] = sentinel
  int32_t valoff[17];          // index of the first symbol of a length minus its first code
  uint8_t vals[256];
};

// counts[1..16], symbols -> canonical code tables; false when the counts do not describe a prefix code
bool build_huff(Huff& h, const uint8_t* counts, const uint8_t* syms, int nsyms) {
  std::memset(h.look, 0, sizeof(h.look));
  std::memset(h.vals, 0, sizeof(h.vals));
  std::memcpy(h.vals, syms, (size_t)nsyms);
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    const int cnt = counts[len - 1];
    h.valoff[len] = k - code;
    if (cnt) {
      if (code + cnt > (1 << len)) return false;          // more codes of this length than the prefix leaves room for
      for (int i = 0; i < cnt; ++i, ++k, ++code)
        if (len <= 9) {
          const int first = code << (9 - len);
          for (int f = 0; f < (1 << (9 - len)); ++f) h.look[first + f] = (uint16_t)((len << 8) | syms[k]);
        }
      h.maxcode[len] = code - 1;
    } else {
      h.maxcode[len] = -1;
    }
    code <<= 1;
  }
  h.maxcode[17] = 0x7fffffff;
  h.defined = true;
  return true;
}

struct Frame {
  int height = 0, width = 0, ncomp = 0;
  int cid[3] = {0, 0, 0}, hs[3] = {0, 0, 0}, vs[3] = {0, 0, 0}, tq[3] = {0, 0, 0};
  int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
  int restart = 0;
  size_t scan = 0;               // first byte of the entropy-coded segment
  uint16_t quant[4][64];
  bool has_quant[4] = {false, false, false, false};
  Huff dc[4], ac[4];
};

struct Reader {
  const uint8_t* p;
  size_t n, pos;
  bool u8(int& v) { if (pos >= n) return false; v = p[pos++]; return true; }
  bool u16(int& v) { if (pos > n || n - pos < 2) return false; v = (p[pos] << 8) | p[pos + 1]; pos += 2; return true; }
};

// Markers up to and including SOS.  -> TAKEN (frame filled, f.scan set) or the refusal.
int parse_headers(const uint8_t* data, size_t len, Frame& f) {
  Reader r{data, len, 0};
  int a, b;
  if (!r.u8(a) || !r.u8(b) || a != 0xFF || b != 0xD8) return MALFORMED;
  bool have_sof = false, adobe = false;
  int adobe_transform = -1;
  for (;;) {
    int m;
    if (!r.u8(m) || m != 0xFF) return MALFORMED;
    do { if (!r.u8(m)) return MALFORMED; } while (m == 0xFF);           // fill bytes
    if (m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) || (m >= 0xCD && m <= 0xCF) || m == 0xCC ||
        m == 0xDC || m == 0xDE || m == 0xDF)
      return UNSUPPORTED;           // progressive / lossless / hierarchical / arithmetic frames, DAC, DNL, DHP, EXP
    if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9) || m < 0xC0 || m == 0xC8) return MALFORMED;   // no place here
    int seg;
    if (!r.u16(seg) || seg < 2 || (size_t)(seg - 2) > r.n - r.pos) return MALFORMED;
    Reader s{data, r.pos + (size_t)(seg - 2), r.pos};
    r.pos = s.n;
    if (m == 0xC0 || m == 0xC1) {
      int prec, nc;
      if (have_sof) return MALFORMED;
      if (!s.u8(prec) || !s.u16(f.height) || !s.u16(f.width) || !s.u8(nc)) return MALFORMED;
      if (prec != 8) return UNSUPPORTED;
      if (f.height < 1 || f.width < 1 || f.height > 65500 || f.width > 65500) return UNSUPPORTED;
      if (nc != 1 && nc != 3) return UNSUPPORTED;
      f.ncomp = nc;
      for (int c = 0; c < nc; ++c) {
        int hv;
        if (!s.u8(f.cid[c]) || !s.u8(hv) || !s.u8(f.tq[c])) return MALFORMED;
        f.hs[c] = hv >> 4; f.vs[c] = hv & 15;
        if (f.hs[c] < 1 || f.hs[c] > 4 || f.vs[c] < 1 || f.vs[c] > 4 || f.tq[c] > 3) return MALFORMED;
      }
      if (s.pos != s.n) return MALFORMED;
      if (nc == 3) {
        const bool l = (f.hs[0] == 1 && f.vs[0] == 1) || (f.hs[0] == 2 && f.vs[0] == 1) || (f.hs[0] == 2 && f.vs[0] == 2);
        if (!l || f.hs[1] != 1 || f.vs[1] != 1 || f.hs[2] != 1 || f.vs[2] != 1) return UNSUPPORTED;
        if (f.cid[0] == f.cid[1] || f.cid[0] == f.cid[2] || f.cid[1] == f.cid[2]) return MALFORMED;
      } else {
        f.hs[0] = f.vs[0] = 1;       // a single-component scan is not interleaved: one block per MCU whatever the factors say
      }
      have_sof = true;
    } else if (m == 0xC4) {
      while (s.pos < s.n) {
        int tc;
        uint8_t counts[16];
        if (!s.u8(tc)) return MALFORMED;
        if ((tc >> 4) > 1 || (tc & 15) > 3) return MALFORMED;
        int total = 0;
        for (int i = 0; i < 16; ++i) { int c; if (!s.u8(c)) return MALFORMED; counts[i] = (uint8_t)c; total += c; }
        if (total > 256 || (size_t)total > s.n - s.pos) return MALFORMED;
        Huff& h = (tc >> 4) ? f.ac[tc & 15] : f.dc[tc & 15];
        h.defined = false;
        if (!build_huff(h, counts, s.p + s.pos, total)) return MALFORMED;
        s.pos += (size_t)total;
      }
    } else if (m == 0xDB) {
      while (s.pos < s.n) {
        int pt;
        if (!s.u8(pt)) return MALFORMED;
        if ((pt & 15) > 3) return MALFORMED;
        if ((pt >> 4) == 1) return UNSUPPORTED;          // 16-bit table
        if ((pt >> 4) != 0) return MALFORMED;
        if (s.n - s.pos < 64) return MALFORMED;
        for (int k = 0; k < 64; ++k) f.quant[pt & 15][kZigzag[k]] = s.p[s.pos + k];
        f.has_quant[pt & 15] = true;
        s.pos += 64;
      }
    } else if (m == 0xDD) {
      if (!s.u16(f.restart) || s.pos != s.n) return MALFORMED;
    } else if (m == 0xEE) {
      if (s.n - s.pos >= 12 && std::memcmp(s.p + s.pos, "Adobe", 5) == 0) { adobe = true; adobe_transform = s.p[s.pos + 11]; }
    } else if (m == 0xDA) {
      int ns;
      if (!have_sof) return MALFORMED;
      if (!s.u8(ns)) return MALFORMED;
      if (ns < 1 || ns > 4) return MALFORMED;
      if (ns != f.ncomp) return UNSUPPORTED;             // one scan of a multi-scan stream
      for (int c = 0; c < ns; ++c) {
        int id, t;
        if (!s.u8(id) || !s.u8(t)) return MALFORMED;
        if (id != f.cid[c]) return UNSUPPORTED;          // components out of frame order
        f.td[c] = t >> 4; f.ta[c] = t & 15;
        if (f.td[c] > 3 || f.ta[c] > 3) return MALFORMED;
        if (!f.dc[f.td[c]].defined || !f.ac[f.ta[c]].defined || !f.has_quant[f.tq[c]]) return MALFORMED;   // a missing table
      }
      int ss, se, ahal;
      if (!s.u8(ss) || !s.u8(se) || !s.u8(ahal) || s.pos != s.n) return MALFORMED;
      if (ss != 0 || se != 63 || ahal != 0) return UNSUPPORTED;
      if (f.ncomp == 3) {
        // libjpeg's colour-space guess: Adobe transform 0, and 'R','G','B' ids without a (well-formed) JFIF segment, mean RGB
        // data, which PIL does not convert.  Such ids are refused whatever APP0 holds.
        if (adobe && adobe_transform != 1) return UNSUPPORTED;
        if (!adobe && f.cid[0] == 'R' && f.cid[1] == 'G' && f.cid[2] == 'B') return UNSUPPORTED;
      }
      f.scan = r.pos;
      return TAKEN;
    }
    // every other APPn / COM / JPGn segment: skipped by its length
  }
}

void fill_geometry(const Frame& f, poem_jpeg_desc_t& d) {
  d.height = f.height; d.width = f.width; d.ncomp = f.ncomp; d.hs = f.hs[0]; d.vs = f.vs[0];
  const int mx = (f.width + 8 * f.hs[0] - 1) / (8 * f.hs[0]), my = (f.height + 8 * f.vs[0] - 1) / (8 * f.vs[0]);
  int64_t blocks = 0;
  for (int c = 0; c < 3; ++c) {
    d.blocks_w[c] = c < f.ncomp ? mx * (c == 0 ? f.hs[0] : 1) : 0;
    d.blocks_h[c] = c < f.ncomp ? my * (c == 0 ? f.vs[0] : 1) : 0;
    blocks += (int64_t)d.blocks_w[c] * d.blocks_h[c];
    if (c < f.ncomp) std::memcpy(d.quant[c], f.quant[f.tq[c]], sizeof(d.quant[c]));
  }
  d.coef_bytes = blocks * 128;
}

// Bit reader over the entropy-coded segment: unstuffs FF 00, stops in front of a marker and never reads past it.
struct Bits {
  const uint8_t* p;
  size_t n, pos;
  uint64_t acc = 0;
  int cnt = 0;
  void fill() {
    while (cnt <= 56 && pos < n) {
      const int b = p[pos];
      if (b == 0xFF) {
        if (pos + 1 >= n || p[pos + 1] != 0x00) return;     // a marker (or the end): the data stops here
        pos += 2;
      } else {
        pos += 1;
      }
      acc = (acc << 8) | (uint64_t)b;
      cnt += 8;
    }
  }
  // the next 16 bits, zero-padded behind the data (what is really there is cnt)
  int peek16() {
    if (cnt < 16) fill();
    return cnt >= 16 ? (int)((acc >> (cnt - 16)) & 0xFFFF) : (int)((acc << (16 - cnt)) & 0xFFFF);
  }
  bool skip(int k) { if (k > cnt) return false; cnt -= k; return true; }
  bool get(int k, int& v) {                                  // k in 1..16
    if (cnt < k) fill();
    if (cnt < k) return false;
    v = (int)((acc >> (cnt - k)) & ((1u << k) - 1));
    cnt -= k;
    return true;
  }
};

inline bool decode_sym(Bits& b, const Huff& h, int& sym) {
  const int w = b.peek16();
  const int e = h.look[w >> 7];
  if (e) { sym = e & 255; return b.skip(e >> 8); }
  int len = 10;
  while (len <= 16 && (w >> (16 - len)) > h.maxcode[len]) ++len;
  if (len > 16) return false;
  const int idx = (w >> (16 - len)) + h.valoff[len];
  if (idx < 0 || idx > 255) return false;
  sym = h.vals[idx];
  return b.skip(len);
}

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// The scan of one image -> its coefficient range.  coef has room for d.coef_bytes (checked by the caller).
int decode_scan(const uint8_t* data, size_t len, const Frame& f, const poem_jpeg_desc_t& d, int16_t* coef) {
  std::memset(coef, 0, (size_t)d.coef_bytes);
  Bits b{data, len, f.scan};
  const int mx = d.blocks_w[f.ncomp - 1], my = d.blocks_h[f.ncomp - 1];      // the chroma (or the only) grid is the MCU grid
  int16_t* plane[3];
  {
    int64_t o = 0;
    for (int c = 0; c < f.ncomp; ++c) { plane[c] = coef + o * 64; o += (int64_t)d.blocks_w[c] * d.blocks_h[c]; }
  }
  int pred[3] = {0, 0, 0};
  int64_t mcu = 0;
  int next_rst = 0;
  for (int y = 0; y < my; ++y) {
    for (int x = 0; x < mx; ++x, ++mcu) {
      if (f.restart && mcu && mcu % f.restart == 0) {
        if (b.cnt >= 8) return MALFORMED;                     // whole bytes between the data and the marker
        b.cnt = 0; b.acc = 0;
        if (b.n - b.pos < 2 || b.p[b.pos] != 0xFF || b.p[b.pos + 1] != 0xD0 + next_rst) return MALFORMED;
        b.pos += 2;
        next_rst = (next_rst + 1) & 7;
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < f.ncomp; ++c) {
        const int nh = c == 0 ? d.hs : 1, nv = c == 0 ? d.vs : 1;
        const Huff& hd = f.dc[f.td[c]];
        const Huff& ha = f.ac[f.ta[c]];
        const uint16_t* q = d.quant[c];
        for (int v = 0; v < nv; ++v)
          for (int h = 0; h < nh; ++h) {
            int16_t* blk = plane[c] + ((int64_t)(y * nv + v) * d.blocks_w[c] + (x * nh + h)) * 64;
            int s, bits;
            if (!decode_sym(b, hd, s)) return MALFORMED;
            if (s > 11) return MALFORMED;
            int diff = 0;
            if (s) { if (!b.get(s, bits)) return MALFORMED; diff = extend(bits, s); }
            pred[c] += diff;
            if (pred[c] < -32768 || pred[c] > 32767) return MALFORMED;
            blk[0] = (int16_t)pred[c];
            int64_t l1 = (int64_t)std::abs(pred[c]) * q[0];
            for (int k = 1; k < 64; ++k) {
              int rs;
              if (!decode_sym(b, ha, rs)) return MALFORMED;
              const int run = rs >> 4, sz = rs & 15;
              if (sz == 0) {
                if (run != 15) break;                          // end of block
                k += 15;
                continue;
              }
              k += run;
              if (k > 63) return MALFORMED;
              if (!b.get(sz, bits)) return MALFORMED;
              const int val = extend(bits, sz);
              const int nat = kZigzag[k];
              blk[nat] = (int16_t)val;                         // |val| < 2^15
              l1 += (int64_t)std::abs(val) * q[nat];
            }
            if (l1 > POEM_JPEG_L1_MAX) return RANGE;
          }
      }
    }
  }
  // the scan must end as the grammar says: at most 7 padding bits, then EOI
  if (b.cnt >= 8) return MALFORMED;
  size_t p = b.pos;
  if (p >= len || data[p] != 0xFF) return MALFORMED;
  while (p < len && data[p] == 0xFF) ++p;
  if (p >= len || data[p] != 0xD9) return MALFORMED;
  return TAKEN;
}

// Headers of all streams of a call -> frames, descs (status, geometry, consecutive 16-byte aligned coef_offsets).  -> the bytes
// that layout needs.  Shared by the serial route and the parallel one: the header-stage refusals are the same by construction.
int64_t layout_headers(const uint8_t* const* streams, const int64_t* lengths, int n, std::vector<Frame>& frames, poem_jpeg_desc_t* descs) {
  int64_t need = 0;
  for (int i = 0; i < n; ++i) {
    poem_jpeg_desc_t& d = descs[i];
    std::memset(&d, 0, sizeof(d));
    d.status = parse_headers(streams[i], (size_t)lengths[i], frames[(size_t)i]);
    if (d.status != TAKEN) continue;
    fill_geometry(frames[(size_t)i], d);
    d.coef_offset = need;
    need += (d.coef_bytes + 15) & ~(int64_t)15;
  }
  return need;
}

// block_base / quad_base over the images taken, and totals[0..3]
void finish_totals(poem_jpeg_desc_t* descs, int n, int64_t need, int64_t* totals) {
  int64_t blocks = 0, quads = 0, taken = 0;
  for (int i = 0; i < n; ++i) {
    poem_jpeg_desc_t& d = descs[i];
    d.block_base = blocks; d.quad_base = quads;
    if (d.status != TAKEN) continue;
    blocks += d.coef_bytes / 128;
    quads += (int64_t)d.height * ((d.width + 3) / 4);
    ++taken;
  }
  totals[0] = need; totals[1] = blocks; totals[2] = quads; totals[3] = taken;
}

// ---- the parallel entropy decoder, host side (csrc/jpeg_entropy.h) ---------------------------------------------------------------
void compact_huff(const Huff& h, poem_jpeg_huff_t& t) {
  std::memset(&t, 0, sizeof(t));
  std::memcpy(t.look, h.look, sizeof(t.look));
  t.maxcode[0] = -1;
  for (int l = 1; l <= 17; ++l) t.maxcode[l] = h.maxcode[l];
  t.valoff[0] = 0;
  for (int l = 1; l <= 16; ++l) t.valoff[l] = h.valoff[l];
  std::memcpy(t.vals, h.vals, sizeof(t.vals));
}

// The distinct tables the scan of a frame names, DC ones first (at most 3 + 3) -> their count; out may be NULL.
int select_tables(const Frame& f, poem_jpeg_huff_t* out, uint8_t* dc_sel, uint8_t* ac_sel) {
  int count = 0, slot_of[2][4];
  for (int cls = 0; cls < 2; ++cls) {
    for (int t = 0; t < 4; ++t) slot_of[cls][t] = -1;
    for (int c = 0; c < f.ncomp; ++c) {
      const int id = cls ? f.ta[c] : f.td[c];
      if (slot_of[cls][id] < 0) {
        if (out) compact_huff(cls ? f.ac[id] : f.dc[id], out[count]);
        slot_of[cls][id] = count++;
      }
      (cls ? ac_sel : dc_sel)[c] = (uint8_t)slot_of[cls][id];
    }
  }
  return count;
}

bool subseq_ok(int s) { return s >= 16 && s <= 1024 && (s & (s - 1)) == 0; }

// One image through the parallel algorithm in plain loops: what a workgroup of csrc/jpeg_entropy.hip does, lane after lane.
// seg: the entropy-coded segment up to the end of the stream.  -> status; rounds: fixed-point rounds taken.
int parallel_scan(const uint8_t* seg, int64_t n, const Frame& f, const poem_jpeg_desc_t& d, int S, int16_t* coef, int32_t& rounds) {
  std::memset(coef, 0, (size_t)d.coef_bytes);
  rounds = 0;
  poem_jpeg_huff_t tabs[6];
  uint8_t dc_sel[3] = {0, 0, 0}, ac_sel[3] = {0, 0, 0};
  select_tables(f, tabs, dc_sel, ac_sel);
  JpegScanCtx c;
  jpeg_scan_geometry(d, c);
  c.data = seg; c.n = n; c.zigzag = kZigzag; c.restart = f.restart;
  for (int k = 0; k < 3; ++k) { c.dc[k] = &tabs[dc_sel[k]]; c.ac[k] = &tabs[ac_sel[k]]; }
  const int64_t nsub = (n + S - 1) / S;
  std::vector<JpegSubState> entry((size_t)nsub), exit_((size_t)nsub), where((size_t)nsub);
  std::vector<int32_t> blocks((size_t)nsub, 0), ev((size_t)nsub, JPEG_EV_RUN);
  std::vector<int64_t> base((size_t)nsub + 1, 0);
  std::vector<uint8_t> cur((size_t)nsub, 1), next((size_t)nsub, 0);
  for (int64_t i = 0; i < nsub; ++i) entry[(size_t)i] = JpegSubState{i * S * 8, 0, 0};
  JpegNoSink none;
  for (bool any = nsub > 0; any;) {
    any = false;
    ++rounds;
    for (int64_t i = 0; i < nsub; ++i) {                       // every lane whose entry changed decodes again, writing nothing
      if (!cur[(size_t)i]) continue;
      JpegSubState st = entry[(size_t)i];
      int done = 0, e = JPEG_EV_RUN;
      if (st.bit >= 0) e = jpeg_sub_decode(c, st, (i + 1) * S * 8, false, done, none);
      if (e != JPEG_EV_RUN) { where[(size_t)i] = st; st = JpegSubState{(i + 1) * S * 8, 0, 0}; }   // an event: the next lane keeps its guess
      exit_[(size_t)i] = st;
      blocks[(size_t)i] = done; ev[(size_t)i] = e;
    }
    for (int64_t i = 0; i < nsub; ++i) {                       // its exit state becomes the next lane's entry
      if (!cur[(size_t)i]) continue;
      cur[(size_t)i] = 0;
      if (i + 1 < nsub && !jpeg_state_eq(exit_[(size_t)i], entry[(size_t)i + 1])) {
        entry[(size_t)i + 1] = exit_[(size_t)i];
        next[(size_t)i + 1] = 1;
        any = true;
      }
    }
    cur.swap(next);
  }
  // the first event of the converged trace (what lies behind it was decoded from guesses and counts for nothing), then the first
  // block of every subsequence
  int event = JPEG_EV_RUN;
  JpegSubState at{0, 0, 0};
  int64_t event_sub = -1;
  for (int64_t i = 0; i < nsub; ++i)
    if (ev[(size_t)i] != JPEG_EV_RUN) { event = ev[(size_t)i]; at = where[(size_t)i]; event_sub = i; break; }
  int64_t sum = 0;
  for (int64_t i = 0; i < nsub; ++i) { base[(size_t)i] = sum; sum += blocks[(size_t)i]; }
  int status = TAKEN;
  for (int64_t i = 0; i < (event_sub >= 0 ? event_sub + 1 : nsub); ++i) {       // the write pass, up to the event
    if (entry[(size_t)i].bit < 0) continue;
    JpegCoefSink sink;
    sink.start(&c, coef, base[(size_t)i]);
    JpegSubState st = entry[(size_t)i];
    int done = 0;
    jpeg_sub_decode(c, st, (i + 1) * S * 8, false, done, sink);
    if (sink.err) status = sink.err;
  }
  const int fin = jpeg_finish(c, event, at, event_sub >= 0 ? base[(size_t)event_sub] + blocks[(size_t)event_sub] : 0, coef);
  if (fin) status = fin;
  if (status) return status;
  // the DC pass: differences -> predictions, per component in MCU order, from zero at every restart interval
  {
    JpegCoefSink walk;
    walk.start(&c, coef, 0);
    int64_t pred[3] = {0, 0, 0};
    for (int64_t mcu = 0; mcu < c.total_mcus; ++mcu) {
      if (c.restart && mcu && mcu % c.restart == 0) pred[0] = pred[1] = pred[2] = 0;
      for (int slot = 0; slot < c.bpm; ++slot, walk.next_block()) {
        const int comp = slot < c.hs * c.vs ? 0 : slot - c.hs * c.vs + 1;
        pred[comp] += walk.blk[0];
        if (pred[comp] < -32768 || pred[comp] > 32767) return MALFORMED;
        walk.blk[0] = (int16_t)pred[comp];
      }
    }
  }
  // the block pass: the range guard
  const int16_t* blk = coef;
  for (int comp = 0; comp < d.ncomp; ++comp)
    for (int64_t b = 0; b < (int64_t)d.blocks_w[comp] * d.blocks_h[comp]; ++b, blk += 64) {
      int64_t l1 = 0;
      for (int k = 0; k < 64; ++k) l1 += (int64_t)std::abs((int)blk[k]) * d.quant[comp][k];
      if (l1 > POEM_JPEG_L1_MAX) return RANGE;
    }
  return TAKEN;
}

}  // namespace

extern "C" {

int poem_jpeg_entropy_prepare(const uint8_t* const* streams, const int64_t* lengths, int n, int subseq, poem_jpeg_desc_t* descs,
                              poem_jpeg_scan_t* scans, poem_jpeg_huff_t* tables, int64_t table_room, uint8_t* packed,
                              int64_t packed_bytes, int64_t* totals) {
  if (!streams || !lengths || !descs || !scans || !totals || n <= 0) return POEM_E_ARG;
  if (subseq == 0) subseq = 64;
  if (!subseq_ok(subseq) || (packed && (!tables || table_room < 0 || packed_bytes < 0))) return POEM_E_ARG;
  if (n > 65535) return POEM_E_UNSUPPORTED;
  if ((uintptr_t)packed & 15) return POEM_E_ARG;
  for (int i = 0; i < n; ++i)
    if (!streams[i] || lengths[i] < 0) return POEM_E_ARG;
  std::vector<Frame> frames;
  try {
    frames.resize((size_t)n);
  } catch (const std::bad_alloc&) {
    return POEM_E_UNSUPPORTED;
  }
  const int64_t need = layout_headers(streams, lengths, n, frames, descs);
  finish_totals(descs, n, need, totals);
  int64_t bytes = 0, ntab = 0, subs = 0, most = 0;
  for (int i = 0; i < n; ++i) {
    poem_jpeg_scan_t& s = scans[i];
    std::memset(&s, 0, sizeof(s));
    s.byte_offset = bytes; s.sub_base = subs; s.table_base = (int32_t)ntab;
    if (descs[i].status != TAKEN) continue;
    const Frame& f = frames[(size_t)i];
    s.byte_count = lengths[i] - (int64_t)f.scan;
    const int64_t ns = (s.byte_count + subseq - 1) / subseq;
    if (ns > 0x7fffffff) return POEM_E_UNSUPPORTED;             // a stream of 32 GiB and more
    s.sub_count = (int32_t)ns;
    s.restart = f.restart;
    s.table_count = select_tables(f, nullptr, s.dc_sel, s.ac_sel);
    bytes += (s.byte_count + 15) & ~(int64_t)15;
    ntab += s.table_count;
    subs += ns;
    if (ns > most) most = ns;
  }
  totals[4] = bytes; totals[5] = ntab; totals[6] = subs; totals[7] = most;
  if (!packed) return POEM_OK;
  if (packed_bytes < bytes || table_room < ntab) return POEM_E_WORKSPACE;
  for (int i = 0; i < n; ++i) {
    const poem_jpeg_scan_t& s = scans[i];
    if (descs[i].status != TAKEN) continue;
    uint8_t dc_sel[3], ac_sel[3];
    select_tables(frames[(size_t)i], tables + s.table_base, dc_sel, ac_sel);
    std::memcpy(packed + s.byte_offset, streams[i] + frames[(size_t)i].scan, (size_t)s.byte_count);
    const int64_t padded = (s.byte_count + 15) & ~(int64_t)15;
    std::memset(packed + s.byte_offset + s.byte_count, 0, (size_t)(padded - s.byte_count));
  }
  return POEM_OK;
}

int poem_jpeg_entropy_parallel_host(const uint8_t* const* streams, const int64_t* lengths, int n, int subseq, poem_jpeg_desc_t* descs,
                                    int16_t* coef, int64_t coef_bytes, int64_t* totals, int32_t* rounds) {
  if (!streams || !lengths || !descs || !totals || n <= 0 || (coef && coef_bytes < 0)) return POEM_E_ARG;
  if (subseq == 0) subseq = 64;
  if (!subseq_ok(subseq)) return POEM_E_ARG;
  if (n > 65535) return POEM_E_UNSUPPORTED;
  if ((uintptr_t)coef & 15) return POEM_E_ARG;
  for (int i = 0; i < n; ++i)
    if (!streams[i] || lengths[i] < 0) return POEM_E_ARG;
  std::vector<Frame> frames;
  try {
    frames.resize((size_t)n);
  } catch (const std::bad_alloc&) {
    return POEM_E_UNSUPPORTED;
  }
  const int64_t need = layout_headers(streams, lengths, n, frames, descs);
  finish_totals(descs, n, need, totals);
  if (rounds) std::memset(rounds, 0, sizeof(int32_t) * (size_t)n);
  if (!coef) return POEM_OK;
  if (coef_bytes < need) return POEM_E_WORKSPACE;
  try {
    for (int i = 0; i < n; ++i) {
      poem_jpeg_desc_t& d = descs[i];
      if (d.status != TAKEN) continue;
      const Frame& f = frames[(size_t)i];
      int32_t r = 0;
      d.status = parallel_scan(streams[i] + f.scan, lengths[i] - (int64_t)f.scan, f, d, subseq, coef + d.coef_offset / 2, r);
      if (rounds) rounds[i] = r;
    }
  } catch (const std::bad_alloc&) {
    return POEM_E_UNSUPPORTED;
  }
  finish_totals(descs, n, need, totals);
  return POEM_OK;
}

int poem_jpeg_entropy_decode(const uint8_t* const* streams, const int64_t* lengths, int n, poem_jpeg_desc_t* descs, int16_t* coef,
                             int64_t coef_bytes, int64_t* totals, int threads) {
  if (!streams || !lengths || !descs || !totals || n <= 0 || (coef && coef_bytes < 0)) return POEM_E_ARG;
  if (n > 65535) return POEM_E_UNSUPPORTED;                     // poem_warp_affine's limit on the views of a call
  if ((uintptr_t)coef & 15) return POEM_E_ARG;
  for (int i = 0; i < n; ++i)
    if (!streams[i] || lengths[i] < 0) return POEM_E_ARG;
  std::vector<Frame> frames;
  try {
    frames.resize((size_t)n);                                   // ~13 KB each: the Huffman tables
  } catch (const std::bad_alloc&) {
    return POEM_E_UNSUPPORTED;
  }
  const int64_t need = layout_headers(streams, lengths, n, frames, descs);
  auto finish = [&]() { finish_totals(descs, n, need, totals); };
  finish();
  if (!coef) return POEM_OK;
  if (coef_bytes < need) return POEM_E_WORKSPACE;
  int nthr = threads <= 0 ? 8 : (threads > 16 ? 16 : threads);
  if (nthr > n) nthr = n;
  std::atomic<int> next(0);
  auto work = [&]() {
    for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) {
      poem_jpeg_desc_t& d = descs[i];
      if (d.status != TAKEN) continue;
      if (d.coef_offset < 0 || d.coef_offset + d.coef_bytes > coef_bytes) { d.status = MALFORMED; continue; }   // (cannot happen)
      d.status = decode_scan(streams[i], (size_t)lengths[i], frames[(size_t)i], d, coef + d.coef_offset / 2);
    }
  };
  if (nthr <= 1) {
    work();
  } else {
    std::vector<std::thread> pool;
    try {
      pool.reserve((size_t)nthr);
      for (int t = 1; t < nthr; ++t) pool.emplace_back(work);
    } catch (...) {
      // no more threads (or memory) to be had: the ones that started and this one share the work
    }
    work();
    for (auto& t : pool) t.join();
  }
  finish();
  return POEM_OK;
}

int poem_jpeg_reconstruct_host(const poem_jpeg_desc_t* descs, const int16_t* coef, int64_t coef_bytes, const int64_t* out_offsets,
                               uint8_t* out, int64_t out_bytes, int n) {
  if (!descs || !coef || !out_offsets || !out || n <= 0 || coef_bytes < 0 || out_bytes < 0) return POEM_E_ARG;
  std::vector<unsigned char> planes;
  for (int i = 0; i < n; ++i) {
    const poem_jpeg_desc_t& d = descs[i];
    if (!jpeg_desc_ok(d)) continue;
    const int64_t blocks = jpeg_desc_blocks(d);
    if (d.coef_offset > coef_bytes || blocks * 128 > coef_bytes - d.coef_offset) continue;
    const int64_t px = (int64_t)d.height * d.width * 3;
    if (out_offsets[i] < 0 || out_offsets[i] > out_bytes || px > out_bytes - out_offsets[i]) continue;
    try {
      planes.assign((size_t)blocks * 64, 0);
    } catch (const std::bad_alloc&) {
      return POEM_E_UNSUPPORTED;
    }
    const unsigned char* plane[3] = {nullptr, nullptr, nullptr};
    int pitch[3] = {0, 0, 0};
    const int16_t* cf = coef + d.coef_offset / 2;
    unsigned char* pl = planes.data();
    for (int c = 0; c < d.ncomp; ++c) {
      plane[c] = pl; pitch[c] = d.blocks_w[c] * 8;
      for (int by = 0; by < d.blocks_h[c]; ++by)
        for (int bx = 0; bx < d.blocks_w[c]; ++bx, cf += 64) {
          int ws[8][8];
          for (int col = 0; col < 8; ++col) {
            int x[8], o[8];
            for (int k = 0; k < 8; ++k) x[k] = (int)cf[k * 8 + col] * (int)d.quant[c][k * 8 + col];
            jpeg_idct_pass(x, o, 11);
            for (int k = 0; k < 8; ++k) ws[k][col] = o[k];
          }
          for (int row = 0; row < 8; ++row) {
            int o[8];
            jpeg_idct_pass(ws[row], o, 18);
            unsigned char* dst = pl + ((int64_t)by * 8 + row) * pitch[c] + bx * 8;
            for (int k = 0; k < 8; ++k) dst[k] = (unsigned char)jpeg_sample(o[k]);
          }
        }
      pl += (int64_t)d.blocks_w[c] * d.blocks_h[c] * 64;
    }
    unsigned char* dst = out + out_offsets[i];
    for (int y = 0; y < d.height; ++y)
      for (int x = 0; x < d.width; ++x, dst += 3) {
        const unsigned rgb = jpeg_pixel(d, plane, pitch, x, y);
        dst[0] = (unsigned char)rgb; dst[1] = (unsigned char)(rgb >> 8); dst[2] = (unsigned char)(rgb >> 16);
      }
  }
  return POEM_OK;
}

}  // extern "C"
