// tests/emu_buscorrect/fuzz_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program that feeds kamd_bus_whitelist_parse (kamd_bus.cpp) malformed whitelist
// texts; built with -fsanitize=address,undefined (Makefile, target wl_fuzz) it is the sanitizer run of the parser.  Hand-written edge cases, then
// every prefix of them, then texts mutated by a fixed integer generator.  The text, the output array and the error buffer are heap blocks of exactly
// the size the parser is told (the text carries no terminating NUL), so a read or write beyond any of them is a report.  Whatever the parser
// answers: count-only and writing mode agree, an accepted list has a length in 1 .. 32 and codes without high bits, a refusal carries a text.
#include "../../include/kallisto_amd.h"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

static int n_ok = 0, n_bad = 0;

static int one(const std::string& s, size_t err_cap, long cap_delta) {
  std::vector<char> text(s.begin(), s.end());   // (exactly s.size() bytes, no NUL behind them)
  std::vector<char> err(err_cap, 'x');
  uint64_t n = 77, n2 = 78;
  int32_t L = -5, L2 = -6;
  const int rc = kamd_bus_whitelist_parse(text.data(), text.size(), nullptr, 0, &n, &L, err_cap ? err.data() : nullptr, err_cap);
  if (rc != 0) {
    ++n_bad;
    if (err_cap > 1 && err[0] == 0) { fprintf(stderr, "refused without a text: \"%s\"\n", s.c_str()); return 1; }
    if (err_cap && memchr(err.data(), 0, err_cap) == nullptr) { fprintf(stderr, "error text not terminated: \"%s\"\n", s.c_str()); return 1; }
    return 0;
  }
  ++n_ok;
  if (n == 0 || L < 1 || L > 32) { fprintf(stderr, "accepted with n = %llu, L = %d: \"%s\"\n", (unsigned long long)n, L, s.c_str()); return 1; }
  const long want_cap = (long)n + cap_delta;
  const uint64_t cap = want_cap < 0 ? 0 : (uint64_t)want_cap;
  std::unique_ptr<uint64_t[]> out(new uint64_t[cap]());   // (cap == 0: a block of no bytes, not NULL, which would mean count-only)
  const int rc2 = kamd_bus_whitelist_parse(text.data(), text.size(), out.get(), cap, &n2, &L2, err.data(), err_cap);
  if ((rc2 == 0) != (cap >= n) || n2 != n || L2 != L) { fprintf(stderr, "the two modes disagree (cap %llu): \"%s\"\n", (unsigned long long)cap, s.c_str()); return 1; }
  if (rc2 == 0 && L < 32)
    for (uint64_t i = 0; i < n; i++)
      if (out[i] >> (2 * L)) { fprintf(stderr, "a code with high bits: \"%s\"\n", s.c_str()); return 1; }
  return 0;
}

int main() {
  const std::vector<std::string> seeds = {
      "", "\n", "\r\n", "\r", "A", "A\n", "a\r\n", "ACGT\nTTTT\n", "ACGT\r\nTTTT\r\n", "ACGT\n\nTTTT\n", "ACGT\n\n\n", "\n\nACGT", "acgt\nAcGt\n", "ACGT\nACGT\n",
      "ACGT\nACG\n", "ACG\nACGT\n", "ACGN\n", "ACGT\nACGU\n", "ACGT \n", " ACGT\n", "ACGT\tACGT\n", "ACGT\rACGT\n", "ACGT\r\r\n", std::string("AC\0GT\n", 6),
      std::string(32, 'T') + "\n" + std::string(32, 'A') + "\n", std::string(33, 'A') + "\n", std::string(32, 'A') + "\n" + std::string(33, 'A'), std::string(5000, 'A'),
      std::string(5000, '\n'), std::string(3000, '\r'), "ACGTACGTACGTACGT\nACGTACGTACGTACGA\r\nacgtacgtacgtacgc", "A\nC\nG\nT\n", "\xff\xfe\n", "ACGT\n\x80"};
  int bad = 0;
  for (const std::string& s : seeds) {
    for (size_t cap : {(size_t)0, (size_t)1, (size_t)2, (size_t)17, (size_t)256})
      for (long d : {0L, -1L, 3L}) bad += one(s, cap, d);
    if (s.size() < 100)
      for (size_t n = 0; n < s.size(); n++) bad += one(s.substr(0, n), 32, 0);
  }
  uint64_t x = 0x243f6a8885a308d3ULL;
  auto next = [&]() { x = x * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(x >> 33); };
  const char alphabet[] = "ACGTacgtACGT\n\n\n\r\r N\t";
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
    bad += one(s, 48, (long)(next() % 3) - 1);
  }
  printf("wl_fuzz: %d accepted, %d refused, %d failures\n", n_ok, n_bad, bad);
  return bad ? 1 : 0;
}
