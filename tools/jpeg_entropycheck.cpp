// The parallel entropy decoder's host driver (poem_jpeg_entropy_parallel_host: poem-v2_amd/csrc/jpeg.cpp over jpeg_entropy.h)
// against the serial decoder (poem_jpeg_entropy_decode), stand-alone and CPU-only:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/jpeg_entropycheck.cpp
//       poem-v2_amd/csrc/jpeg.cpp -o jpeg_entropycheck -lpthread
//   ./jpeg_entropycheck a.jpg b.jpg ...
// Every stream is decoded as it is, cut at every byte offset, and put through a seeded set of mutations (most of them inside the
// scan), each at subsequence sizes 16 and 128.  The streams live in heap blocks of exactly their length and the coefficients in
// blocks of exactly the size asked for, so a read past a stream or a store past a buffer is the sanitizers' to report.  A case
// passes when the driver returns the serial decoder's verdict (taken / refused; the header-stage code itself where the headers
// refuse), the serial decoder's coefficient bytes where taken, and a round count of at most the number of subsequences.
// Exit status 0 only if every case passed and the files themselves were taken.
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

long cases = 0, taken = 0, refused = 0, max_rounds = 0;

// -> status of the image (0..3), or -1 when the two decoders disagree or the library misbehaved
int run_case(const uint8_t* data, size_t len) {
  uint8_t* own = (uint8_t*)std::malloc(len ? len : 1);
  if (len) std::memcpy(own, data, len);
  const uint8_t* streams[1] = {own};
  const int64_t lengths[1] = {(int64_t)len};
  poem_jpeg_desc_t ref;
  int64_t totals[4];
  int status = -1;
  ++cases;
  int16_t* ref_coef = nullptr;
  int64_t need = 0;
  if (poem_jpeg_entropy_decode(streams, lengths, 1, &ref, nullptr, 0, totals, 1) == POEM_OK && ref.status >= 0 && ref.status <= 3) {
    status = ref.status;
    need = totals[0];
    if (status == 0) {
      if (need <= 0 || need % 16) { std::free(own); return -1; }
      ref_coef = (int16_t*)std::aligned_alloc(16, (size_t)need);
      if (poem_jpeg_entropy_decode(streams, lengths, 1, &ref, ref_coef, need, totals, 1) != POEM_OK) status = -1;
      else status = ref.status;
    }
  }
  for (int pass = 0; pass < 2 && status >= 0; ++pass) {
    const int subseq = pass ? 128 : 16;
    poem_jpeg_desc_t d;
    int64_t t2[4];
    int32_t rounds = -1;
    if (poem_jpeg_entropy_parallel_host(streams, lengths, 1, subseq, &d, nullptr, 0, t2, &rounds) != POEM_OK) { status = -1; break; }
    if (ref_coef == nullptr) {                                         // refused by the headers: the same code, and nothing to decode
      if (d.status != ref.status) status = -1;
      continue;
    }
    if (d.status != 0 || t2[0] != need) { status = -1; break; }
    int16_t* coef = (int16_t*)std::aligned_alloc(16, (size_t)need);
    if (poem_jpeg_entropy_parallel_host(streams, lengths, 1, subseq, &d, coef, need - 16, t2, &rounds) != POEM_E_WORKSPACE) status = -1;
    else if (poem_jpeg_entropy_parallel_host(streams, lengths, 1, subseq, &d, coef, need, t2, &rounds) != POEM_OK) status = -1;
    else if ((d.status == 0) != (ref.status == 0) || d.status < 0 || d.status > 3) status = -1;
    else if (d.status == 0 && std::memcmp(coef, ref_coef, (size_t)need) != 0) status = -1;
    else {
      const int64_t scan_bytes_bound = (int64_t)len;                   // the segment is no longer than the stream
      if (rounds < 0 || rounds > (scan_bytes_bound + subseq - 1) / subseq) status = -1;
      if (rounds > max_rounds) max_rounds = rounds;
    }
    std::free(coef);
  }
  std::free(ref_coef);
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
    if (run_case(data.data(), data.size()) != 0) { std::fprintf(stderr, "%s: not taken as it is\n", argv[a]); ++bad; }
    for (size_t cut = 0; cut < data.size(); ++cut)
      if (run_case(data.data(), cut) < 0) { std::fprintf(stderr, "%s: cut at %zu\n", argv[a], cut); ++bad; }
    size_t scan = 0;                                                    // the first SOS: the scan lies behind it
    for (size_t i = 0; i + 1 < data.size(); ++i)
      if (data[i] == 0xFF && data[i + 1] == 0xDA) { scan = i; break; }
    for (int m = 0; m < 3000; ++m) {
      std::vector<uint8_t> mut(data);
      const int edits = (m & 1) ? 1 : 2 + (int)(rnd() % 3);
      for (int e = 0; e < edits; ++e) {
        const bool in_scan = (m % 4) != 3 && scan + 14 < mut.size();     // three in four aimed at the entropy-coded bytes
        const size_t lo = in_scan ? scan + 14 : 0, span = mut.size() - lo;
        const size_t at = lo + rnd() % span;
        switch (rnd() % 6) {
          case 0: mut[at] = (uint8_t)rnd(); break;
          case 1: mut[at] ^= (uint8_t)(1u << (rnd() % 8)); break;
          case 2: mut[at] = 0xFF; break;
          case 3: mut[at] = (uint8_t)(0xD0 + rnd() % 10); break;         // a restart marker's (or EOI's) second byte
          case 4: mut[at] = 0x00; break;
          default: mut[at] = (uint8_t)(mut[at] + 1); break;
        }
      }
      if (run_case(mut.data(), mut.size()) < 0) { std::fprintf(stderr, "%s: mutation %d\n", argv[a], m); ++bad; }
    }
  }
  std::printf("jpeg_entropycheck: %ld cases, %ld taken, %ld refused, most rounds %ld, %d bad\n", cases, taken, refused, max_rounds, bad);
  return bad ? 1 : 0;
}
