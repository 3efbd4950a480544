// Robustness check of the host half of the JPEG route (poem-v2_amd/csrc/jpeg.cpp + jpeg.h), stand-alone and CPU-only:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/jpeg_hostcheck.cpp
//       poem-v2_amd/csrc/jpeg.cpp -o jpeg_hostcheck -lpthread           (or the same line through `hipcc -x c++`)
//   ./jpeg_hostcheck a.jpg b.jpg ...
// Every stream is decoded as it is, cut at every byte offset, and put through a seeded set of single- and multi-byte mutations
// (half of them aimed at the marker segments in front of the scan).  Each case runs poem_jpeg_entropy_decode (size query, then
// the decode into a buffer of exactly the size asked for) and, when the image is taken, poem_jpeg_reconstruct_host into a pixel
// buffer of exactly h * w * 3 bytes; the streams live in heap blocks of exactly their length.  So any read past a stream or write
// past a buffer is the sanitizers' to report.  Exit status 0 only if every case came back as POEM_OK with the image either taken
// or refused (status 1..3) and the files themselves were taken.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "poem_hip.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

long cases = 0, taken = 0, refused = 0;

// -> status of the image (0..3), or -1 when the library misbehaved
int run_case(const uint8_t* data, size_t len, int threads) {
  uint8_t* own = (uint8_t*)std::malloc(len ? len : 1);                 // exactly `len` bytes: an over-read is out of bounds
  if (len) std::memcpy(own, data, len);
  const uint8_t* streams[1] = {own};
  const int64_t lengths[1] = {(int64_t)len};
  poem_jpeg_desc_t desc;
  int64_t totals[4];
  int status = -1;
  ++cases;
  if (poem_jpeg_entropy_decode(streams, lengths, 1, &desc, nullptr, 0, totals, threads) == POEM_OK && desc.status >= 0 &&
      desc.status <= 3) {
    status = desc.status;
    if (status == 0) {
      const int64_t need = totals[0];
      if (need <= 0 || need % 16) { std::free(own); return -1; }
      int16_t* coef = (int16_t*)std::aligned_alloc(16, (size_t)need);
      if (poem_jpeg_entropy_decode(streams, lengths, 1, &desc, coef, need - 16, totals, threads) != POEM_E_WORKSPACE) status = -1;
      else if (poem_jpeg_entropy_decode(streams, lengths, 1, &desc, coef, need, totals, threads) != POEM_OK) status = -1;
      else if (desc.status < 0 || desc.status > 3) status = -1;
      else status = desc.status;
      if (status == 0) {
        const int64_t px = (int64_t)desc.height * desc.width * 3, off = 0;
        uint8_t* out = (uint8_t*)std::malloc((size_t)px);
        if (poem_jpeg_reconstruct_host(&desc, coef, need, &off, out, px, 1) != POEM_OK) status = -1;
        std::free(out);
      }
      std::free(coef);
    }
  }
  std::free(own);
  if (status == 0) ++taken; else if (status > 0) ++refused;
  return status;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s FILE.jpg ...\n", argv[0]); return 2; }
  int bad = 0;
  for (int a = 1; a < argc; ++a) {
    std::FILE* f = std::fopen(argv[a], "rb");
    if (!f) { std::fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
    std::vector<uint8_t> data;
    uint8_t chunk[4096];
    for (size_t n; (n = std::fread(chunk, 1, sizeof(chunk), f)) > 0;) data.insert(data.end(), chunk, chunk + n);
    std::fclose(f);
    if (run_case(data.data(), data.size(), 1) != 0) { std::fprintf(stderr, "%s: not taken as it is\n", argv[a]); ++bad; }
    for (size_t cut = 0; cut < data.size(); ++cut)
      if (run_case(data.data(), cut, 1) < 0) { std::fprintf(stderr, "%s: cut at %zu\n", argv[a], cut); ++bad; }
    size_t scan = 0;                                                    // the first SOS: what lies in front are the marker segments
    for (size_t i = 0; i + 1 < data.size(); ++i)
      if (data[i] == 0xFF && data[i + 1] == 0xDA) { scan = i; break; }
    for (int m = 0; m < 3000; ++m) {
      std::vector<uint8_t> mut(data);
      const int edits = (m & 1) ? 1 : 2 + (int)(rnd() % 7);
      for (int e = 0; e < edits; ++e) {
        const size_t span = ((m >> 1) & 1) && scan ? scan + 16 : mut.size();
        const size_t at = rnd() % (span < mut.size() ? span : mut.size());
        switch (rnd() % 4) {
          case 0: mut[at] = (uint8_t)rnd(); break;
          case 1: mut[at] ^= (uint8_t)(1u << (rnd() % 8)); break;
          case 2: mut[at] = 0xFF; break;
          default: mut[at] = (uint8_t)(mut[at] + 1); break;
        }
      }
      if (run_case(mut.data(), mut.size(), 1 + (m % 3 == 0)) < 0) { std::fprintf(stderr, "%s: mutation %d\n", argv[a], m); ++bad; }
    }
  }
  std::printf("jpeg_hostcheck: %ld cases, %ld taken, %ld refused, %d bad\n", cases, taken, refused, bad);
  return bad ? 1 : 0;
}
