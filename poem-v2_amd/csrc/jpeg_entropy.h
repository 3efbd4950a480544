// The per-subsequence Huffman decode step of the parallel entropy decoder (include/poem_hip.h "baseline JPEG",
// poem_jpeg_entropy_device / poem_jpeg_entropy_parallel_host): bit reader, state machine and checks, shared by the plain-loop host
// driver (csrc/jpeg.cpp) and the kernels (csrc/jpeg_entropy.hip) as csrc/jpeg.h is for the arithmetic.  It restates decode_scan of
// csrc/jpeg.cpp (the serial decoder, the yardstick) as a pure function of a small STATE, so that a scan can be decoded piecewise:
//
//   state   = (bit, slot, k, m): raw bit position of the next symbol in the entropy-coded segment (stuffing bytes counted, never
//             pointing at one), block slot inside the MCU, zig-zag index (0: a DC symbol is due), MCUs since the last restart
//             marker (always 0 without DRI).
//   step    = jpeg_sub_decode: symbols from `st` while they START in front of `end_bit`; returns JPEG_EV_RUN with the state at the
//             first symbol at or behind end_bit, or an EVENT that ends the decode of the image at this point.  A lane that meets an
//             event hands nothing on (its successor keeps its guess); the FIRST event in stream order is the serial decoder's.
//
// Byte stuffing is handled in the reader, not compacted away: positions stay positions of the stream as uploaded, a subsequence
// is a fixed byte range, and no pre-pass has to touch the bytes.  The reader keeps, beside the 64-bit window of data bits, a mask of
// the bits that end a stuffed FF: consuming across one adds the 8 bits of its 00 to the raw position.
//
// What only the ABSOLUTE MCU index can decide is not decided here but handed back as an event (a lane that starts from a guessed
// state does not know how many MCUs lie in front of it):
//   JPEG_EV_STOP      at the start of an MCU fewer than 8 data bits remain in front of a marker (or the end of the bytes).  The serial
//                     decoder stops here if this was the last MCU, and otherwise goes on into the zero padding (and is refused
//                     unless whole MCUs fit into those < 8 bits): jpeg_finish decides, and runs that tail itself, serially.
//   JPEG_EV_NEED_RST  the restart interval is full and no RSTn stands where it must: fine if this was the last MCU, refused otherwise.
// A restart marker is taken where the interval is full (m == restart) and `FF D0..D7` follows fewer than 8 unread bits; its NUMBER
// (mod 8) needs the absolute index too and is checked by passes that know it (Sink::abs_blocks() >= 0).
#ifndef POEM_JPEG_ENTROPY_H
#define POEM_JPEG_ENTROPY_H

#include <stdint.h>
#include "../../include/poem_hip.h"
#include "jpeg.h"

enum { JPEG_EV_RUN = 0, JPEG_EV_UNSUPPORTED = 1, JPEG_EV_MALFORMED = 2, JPEG_EV_RANGE = 3, JPEG_EV_STOP = 4, JPEG_EV_NEED_RST = 5,
       JPEG_EV_DONE = 6 };

struct JpegSubState {
  long long bit;                 // raw bit position in the segment
  int slot_k;                    // slot << 8 | k
  int m;                         // MCUs since the last restart marker (0 without DRI)
};
POEM_JPEG_HD bool jpeg_state_eq(const JpegSubState& a, const JpegSubState& b) {
  return a.bit == b.bit && a.slot_k == b.slot_k && a.m == b.m;
}

// What a lane needs of one image.  `data` is the entropy-coded segment up to the END of the stream (n bytes).
struct JpegScanCtx {
  const unsigned char* data;
  long long n;
  const poem_jpeg_huff_t* dc[3];
  const poem_jpeg_huff_t* ac[3];
  const unsigned char* zigzag;   // 64 entries
  int ncomp, hs, vs, bpm;        // blocks per MCU: hs * vs + (ncomp - 1)
  int restart;
  int mx;                        // MCUs per row
  long long total_blocks, total_mcus;
  int blocks_w[3];
  long long plane_off[3];        // first coefficient of each component's plane (in int16 elements)
};

template <class D>
POEM_JPEG_HD void jpeg_scan_geometry(const D& d, JpegScanCtx& c) {
  c.ncomp = d.ncomp; c.hs = d.ncomp == 3 ? d.hs : 1; c.vs = d.ncomp == 3 ? d.vs : 1;
  c.bpm = c.hs * c.vs + (d.ncomp - 1);
  c.mx = d.blocks_w[d.ncomp - 1];
  c.total_mcus = (long long)d.blocks_w[d.ncomp - 1] * d.blocks_h[d.ncomp - 1];
  c.total_blocks = c.total_mcus * c.bpm;
  long long o = 0;
  for (int k = 0; k < 3; ++k) {
    c.blocks_w[k] = k < d.ncomp ? d.blocks_w[k] : 0;
    c.plane_off[k] = o * 64;
    if (k < d.ncomp) o += (long long)d.blocks_w[k] * d.blocks_h[k];
  }
}
// The geometry the state machine relies on: the luma grid is the chroma grid times the sampling factors (what fill_geometry
// produces; a descriptor read back from device memory is checked before it is trusted).
template <class D>
POEM_JPEG_HD bool jpeg_scan_desc_ok(const D& d) {
  if (!jpeg_desc_ok(d)) return false;
  if (d.ncomp == 3)
    return d.blocks_w[0] == d.blocks_w[2] * d.hs && d.blocks_h[0] == d.blocks_h[2] * d.vs && d.blocks_w[1] == d.blocks_w[2] &&
           d.blocks_h[1] == d.blocks_h[2];
  return true;
}

POEM_JPEG_HD int jpeg_byte(const JpegScanCtx& c, long long i) {          // i in [0, c.n)
  return c.data[i];
}

// ---- the bit reader -----------------------------------------------------------------------------------------------------------
struct JpegBits {
  const JpegScanCtx* c;
  long long n, rp;               // rp: next raw byte to load
  unsigned long long acc, sacc;  // data bits; sacc: 1 where a bit is the last of a stuffed FF
  int cnt;                       // real data bits in acc
  long long bit;                 // raw position of the next unconsumed bit

  POEM_JPEG_HD int at(long long i) const { return jpeg_byte(*c, i); }
  POEM_JPEG_HD void start(const JpegScanCtx& ctx, long long at) {
    c = &ctx; n = ctx.n; bit = at; acc = 0; sacc = 0; cnt = 0;
    rp = at >> 3;
    const int off = (int)(at & 7);
    if (off && rp < n) {                                   // inside a byte: a true state only (guesses sit on whole bytes)
      const int b = this->at(rp);
      if (b == 0xFF) {
        if (rp + 1 < n && this->at(rp + 1) == 0x00) { acc = (unsigned)b & ((1u << (8 - off)) - 1); sacc = 1; cnt = 8 - off; rp += 2; }
      } else {
        acc = (unsigned)b & ((1u << (8 - off)) - 1); cnt = 8 - off; rp += 1;
      }
    }
  }
  POEM_JPEG_HD void fill() {
    while (cnt <= 32 && rp < n) {                           // (a few bytes per call: lanes of a wave wait for the longest fill)
      const int b = at(rp);
      if (b == 0xFF) {
        if (rp + 1 >= n || at(rp + 1) != 0x00) return;      // a marker (or the end): the data stops here
        rp += 2;
        sacc = (sacc << 8) | 1ull;
      } else {
        rp += 1;
        sacc <<= 8;
      }
      acc = (acc << 8) | (unsigned long long)b;
      cnt += 8;
    }
  }
  POEM_JPEG_HD int peek16() {
    if (cnt < 16) fill();
    return cnt >= 16 ? (int)((acc >> (cnt - 16)) & 0xFFFF) : (int)((acc << (16 - cnt)) & 0xFFFF);
  }
  POEM_JPEG_HD void consume(int k) {                        // k <= cnt, k in 1..16
    const unsigned crossed = (unsigned)((sacc >> (cnt - k)) & ((1u << k) - 1));
#if defined(__HIP_DEVICE_COMPILE__)
    const int stuffed = __popc(crossed);
#else
    const int stuffed = __builtin_popcount(crossed);
#endif
    bit += k + 8 * stuffed;
    cnt -= k;
  }
  POEM_JPEG_HD bool skip(int k) { if (k > cnt) return false; consume(k); return true; }
  POEM_JPEG_HD bool get(int k, int& v) {
    if (cnt < k) fill();
    if (cnt < k) return false;
    v = (int)((acc >> (cnt - k)) & ((1u << k) - 1));
    consume(k);
    return true;
  }
};

POEM_JPEG_HD bool jpeg_decode_sym(JpegBits& b, const poem_jpeg_huff_t& h, int& sym) {
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

POEM_JPEG_HD int jpeg_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// ---- sinks ------------------------------------------------------------------------------------------------------------------------
// A sink receives the coefficients of the block in progress.  The fixed-point rounds use JpegNoSink: nothing is written and nothing
// absolute is known.
struct JpegNoSink {
  POEM_JPEG_HD long long abs_blocks() const { return -1; }
  POEM_JPEG_HD void put(int, int, int) {}
  POEM_JPEG_HD void next_block() {}
  POEM_JPEG_HD void flag(int) {}
};

// Stores into the image's own coefficient range: block index -> (component, row, column) through the MCU order, every store
// bounded by the image's block count.  DC DIFFERENCES go to element 0 (the DC pass turns them into predictions).
struct JpegCoefSink {
  const JpegScanCtx* c;
  int16_t* coef;                 // the image's range
  long long b;                   // index (in scan order) of the block in progress
  long long mcu;
  int err;
  int16_t* blk;

  POEM_JPEG_HD void seek(int slot) {
    blk = nullptr;
    if (b < 0 || b >= c->total_blocks) return;
    const long long y = mcu / c->mx, x = mcu % c->mx;
    const int luma = c->hs * c->vs;
    int comp = 0, v = 0, h = 0, nh = c->hs, nv = c->vs;
    if (slot < luma) { v = slot / c->hs; h = slot % c->hs; } else { comp = slot - luma + 1; nh = nv = 1; }
    if (comp >= c->ncomp) return;
    blk = coef + c->plane_off[comp] + ((y * nv + v) * c->blocks_w[comp] + (x * nh + h)) * 64;
  }
  POEM_JPEG_HD void start(const JpegScanCtx* ctx, int16_t* range, long long block) {
    c = ctx; coef = range; b = block; err = 0;
    mcu = block / ctx->bpm;
    seek((int)(block % ctx->bpm));
  }
  POEM_JPEG_HD long long abs_blocks() const { return b; }
  POEM_JPEG_HD void put(int, int nat, int val) { if (blk) blk[nat] = (int16_t)val; else err = JPEG_EV_MALFORMED; }
  POEM_JPEG_HD void next_block() {
    ++b;
    const int slot = (int)(b % c->bpm);
    if (slot == 0) ++mcu;
    seek(slot);
  }
  POEM_JPEG_HD void flag(int e) { if (!err) err = e; }
};

// ---- the step ---------------------------------------------------------------------------------------------------------------------
// Decodes from `st` (not dead) the symbols that start in front of end_bit.  tail: the absolute MCU index is known (sink.abs_blocks()),
// the scan ends at total_mcus (JPEG_EV_DONE; st.bit is where the serial decoder stands) and a STOP never happens.
// -> event; `blocks` += blocks completed.  On JPEG_EV_RUN st is the exit state; on STOP / NEED_RST / DONE st.bit is the position
// reached (and st.m the interval count on STOP); on a refusal st is unspecified.
template <class Sink>
POEM_JPEG_HD int jpeg_sub_decode(const JpegScanCtx& c, JpegSubState& st, long long end_bit, bool tail, int& blocks, Sink& sink) {
  JpegBits b;
  b.start(c, st.bit);
  int slot = st.slot_k >> 8, k = st.slot_k & 255, m = st.m;
  if (slot < 0 || slot >= c.bpm || k > 63) return JPEG_EV_MALFORMED;
  for (;;) {
    if (b.bit >= end_bit) {
      st.bit = b.bit; st.slot_k = (slot << 8) | k; st.m = m;
      return JPEG_EV_RUN;
    }
    const int comp = slot < c.hs * c.vs ? 0 : slot - c.hs * c.vs + 1;
    if (k == 0) {
      if (slot == 0) {                                                  // the start of an MCU
        const long long done = sink.abs_blocks();
        if (tail && done >= c.total_blocks) {
          st.bit = b.bit;
          return JPEG_EV_DONE;
        }
        if (c.restart && m == c.restart) {
          b.fill();
          if (b.cnt >= 8) return JPEG_EV_MALFORMED;                     // whole bytes between the data and the marker
          const long long nb = b.rp;                                    // fill() stopped here: the end, or FF and not 00
          const int mark = nb + 1 < c.n && jpeg_byte(c, nb) == 0xFF ? jpeg_byte(c, nb + 1) : 0;
          if ((mark & 0xF8) == 0xD0) {
            if (done >= 0) {                                            // the marker's number: RST0 closes the first interval
              const long long intervals = done / c.bpm / c.restart;
              if ((mark & 7) != (int)((intervals - 1) & 7)) sink.flag(JPEG_EV_MALFORMED);
            }
            b.start(c, (nb + 2) * 8);
            m = 0;
            continue;
          }
          if (tail) return JPEG_EV_MALFORMED;
          st.bit = b.bit;
          return JPEG_EV_NEED_RST;
        }
        if (!tail) {
          b.fill();
          if (b.cnt < 8) { st.bit = b.bit; st.m = m; return JPEG_EV_STOP; }
        }
      }
      int s, bits;
      if (!jpeg_decode_sym(b, *c.dc[comp], s)) return JPEG_EV_MALFORMED;
      if (s > 11) return JPEG_EV_MALFORMED;
      if (s) {
        if (!b.get(s, bits)) return JPEG_EV_MALFORMED;
        sink.put(comp, 0, jpeg_extend(bits, s));
      }
      k = 1;
      continue;
    }
    int rs, bits;
    bool end_of_block = false;
    if (!jpeg_decode_sym(b, *c.ac[comp], rs)) return JPEG_EV_MALFORMED;
    const int run = rs >> 4, sz = rs & 15;
    if (sz == 0) {
      if (run != 15) end_of_block = true;
      else k += 16;                                                     // ZRL; carrying k past 63 just ends the block
    } else {
      k += run;
      if (k > 63) return JPEG_EV_MALFORMED;
      if (!b.get(sz, bits)) return JPEG_EV_MALFORMED;
      sink.put(comp, c.zigzag[k], jpeg_extend(bits, sz));
      ++k;
    }
    if (end_of_block || k > 63) {
      ++blocks;
      sink.next_block();
      k = 0;
      if (++slot == c.bpm) { slot = 0; if (c.restart) ++m; }
    }
  }
}

// Where the data stops behind position `bit`, if fewer than 8 unread data bits lie in front of that byte; -1 otherwise.
POEM_JPEG_HD long long jpeg_data_end(const JpegScanCtx& c, long long bit) {
  JpegBits b;
  b.start(c, bit);
  b.fill();
  return b.cnt >= 8 ? -1 : b.rp;
}

// The scan must end as the grammar says: fewer than 8 unread bits, then FF.. D9.
POEM_JPEG_HD int jpeg_check_eoi(const JpegScanCtx& c, long long bit) {
  long long nb = jpeg_data_end(c, bit);
  if (nb < 0 || nb >= c.n || jpeg_byte(c, nb) != 0xFF) return JPEG_EV_MALFORMED;
  while (nb < c.n && jpeg_byte(c, nb) == 0xFF) ++nb;
  if (nb >= c.n || jpeg_byte(c, nb) != 0xD9) return JPEG_EV_MALFORMED;
  return 0;
}

// After the fixed point and the write pass: the one event of the converged trace (ev, with the state it left and the blocks
// completed in front of it) -> the image's status (0 taken, 2 malformed).  A STOP short of the frame's block count is where the
// serial decoder reads on into the last (< 8) bits: that tail is decoded here, serially, with the absolute index known, storing
// like the write pass.  It ends within those bits in all but contrived streams (a restart marker taken inside the tail lets it run
// on, still serially: slow, and still the serial decoder's result).
POEM_JPEG_HD int jpeg_finish(const JpegScanCtx& c, int ev, const JpegSubState& at, long long blocks_done, int16_t* coef) {
  if (ev == JPEG_EV_RUN) return JPEG_EV_MALFORMED;                        // the bytes ran out without an end
  if (ev != JPEG_EV_STOP && ev != JPEG_EV_NEED_RST) return ev;            // a refusal
  if (blocks_done == c.total_blocks) return jpeg_check_eoi(c, at.bit);
  if (blocks_done > c.total_blocks || ev == JPEG_EV_NEED_RST) return JPEG_EV_MALFORMED;
  JpegSubState st = at;
  st.slot_k = 0;
  JpegCoefSink sink;
  sink.start(&c, coef, blocks_done);
  int more = 0;
  const int e = jpeg_sub_decode(c, st, (long long)1 << 62, true, more, sink);
  if (e != JPEG_EV_DONE) return JPEG_EV_MALFORMED;
  if (sink.err) return sink.err;
  return jpeg_check_eoi(c, st.bit);
}

#endif  // POEM_JPEG_ENTROPY_H
