// tests/emu_bustag/fuzz_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program that feeds kamd_bus_layout_parse (kamd_bus.cpp) malformed technology strings;
// built with -fsanitize=address,undefined (Makefile, target parse_fuzz) it is the sanitizer run of the parser.  Hand-written edge cases, then every
// prefix of them, then strings mutated by a fixed integer generator.  Whatever the parser answers, an accepted layout must pass the layout check and a
// refusal must carry a text; the error buffer is deliberately small and exactly sized.
#include "../../kallisto_amd/csrc/kamd_bustag.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static int n_ok = 0, n_bad = 0;

static int one(const std::string& s, size_t cap) {
  std::vector<char> err(cap, 'x');   // (heap, exactly cap bytes: a write beyond it is an ASan report)
  kamd_bus_layout L;
  int32_t strand = -7;
  const int rc = kamd_bus_layout_parse(s.c_str(), &L, &strand, cap ? err.data() : nullptr, cap);
  if (rc == 0) {
    ++n_ok;
    char why[64];
    if (kamd::bus_layout_check(&L, why, sizeof why) != 0) { fprintf(stderr, "accepted but fails the check: \"%s\": %s\n", s.c_str(), why); return 1; }
    if (strand < 0 || strand > 2) { fprintf(stderr, "accepted without a strand: \"%s\"\n", s.c_str()); return 1; }
    if (kamd_bus_seq_max_len(&L, 100) < 1) { fprintf(stderr, "no sequence bound: \"%s\"\n", s.c_str()); return 1; }
  } else {
    ++n_bad;
    if (cap > 1 && err[0] == 0) { fprintf(stderr, "refused without a text: \"%s\"\n", s.c_str()); return 1; }
    if (cap && memchr(err.data(), 0, cap) == nullptr) { fprintf(stderr, "error text not terminated: \"%s\"\n", s.c_str()); return 1; }
  }
  return 0;
}

int main() {
  const std::vector<std::string> seeds = {
      "", ":", "::", ":::", "::::", "0,0,16:0,16,28:1,0,0", "10xv3", "10XV3", "VASA-SEQ", "vasa-seq", "BULK", "SMARTSEQ3", "storm-seq", "10XV1",
      "0,0,16:0,16,28", "0,0,16", "0,0,16:0,16,28:1,0,0:2,0,0", "0,0:0,16,28:1,0,0", "0,0,16,:0,16,28:1,0,0", ",0,0,16:0,16,28:1,0,0", "0,,16:0,16,28:1,0,0",
      "a,b,c:0,16,28:1,0,0", "0,0,16:x:1,0,0", "0,0,16:RX:1,0,0", "-2,0,16:0,16,28:1,0,0", "0,-1,16:0,16,28:1,0,0", "0,16,16:0,16,28:1,0,0", "0,16,8:0,16,28:1,0,0",
      "-1,-1,-1:0,0,10:1,0,0", "0,0,8:-1,-1,-1:1,0,0", "-1,-1,-1:-1,-1,-1:0,0,0", "0,0,8:0,8,16:-1,-1,-1", "0,0,8,-1,-1,-1:0,8,16:1,0,0", "2,0,8:0,8,16:1,0,0",
      "0,0,8:0,8,16:0,0,0,1,0,0", "0,0,40:0,40,50:1,0,0", "0,0,0:0,0,0:1,0,0", "0,0,8:0,8,0:1,0,0", "99999999999999999999,0,8:0,8,16:1,0,0", "0,0,2147483647:0,8,16:1,0,0",
      "0,2147483647,0:0,8,16:1,0,0", " 0, 0, 16 : 0,16,28:1,0,0", "0,0,16abc:0,16,28:1,0,0", "+0,+0,+16:0,16,28:1,0,0", "0,0,16:0,16,28:1,0,0\n",
      "0,0,1,0,1,2,0,2,3,0,3,4,0,4,5,0,5,6,0,6,7,0,7,8:0,8,16:1,0,0", "0,0,1,0,1,2,0,2,3,0,3,4,0,4,5,0,5,6,0,6,7,0,7,8,0,8,9:0,9,16:1,0,0",
      std::string(5000, ','), std::string(5000, ':'), std::string(3000, '9'), "0,0,16:0,16,28:1,0,0" + std::string(4000, ' ')};
  int bad = 0;
  for (const std::string& s : seeds) {
    for (size_t cap : {(size_t)0, (size_t)1, (size_t)2, (size_t)17, (size_t)256}) bad += one(s, cap);
    if (s.size() < 100)
      for (size_t n = 0; n < s.size(); n++) bad += one(s.substr(0, n), 32);
  }
  uint64_t x = 0x243f6a8885a308d3ULL;
  auto next = [&]() { x = x * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(x >> 33); };
  const char alphabet[] = "0123456789,,,:::--+ xRX\t";
  for (int it = 0; it < 20000; it++) {
    std::string s = seeds[next() % seeds.size()];
    if (s.size() > 200) s.resize(200);
    const int n_mut = 1 + (int)(next() % 4);
    for (int m = 0; m < n_mut; m++) {
      const char c = alphabet[next() % (sizeof alphabet - 1)];
      const uint32_t how = next() % 3;
      const size_t at = s.empty() ? 0 : next() % (s.size() + 1);
      if (how == 0 || s.empty()) s.insert(s.begin() + at, c);
      else if (how == 1) s[at % s.size()] = c;
      else s.erase(s.begin() + at % s.size());
    }
    bad += one(s, 48);
  }
  printf("parse_fuzz: %d accepted, %d refused, %d failures\n", n_ok, n_bad, bad);
  return bad ? 1 : 0;
}
