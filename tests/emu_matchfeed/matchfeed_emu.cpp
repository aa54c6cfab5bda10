// tests/emu_matchfeed/matchfeed_emu.cpp -- TEST INFRASTRUCTURE: kernel A's item feed (kamd_core.h ItemFeed, the functions k_match_v3 calls) on the CPU.
// W emulated wavefronts take the positions [0, n) of one launch from ONE plain counter in a seeded random interleaving.  A wavefront's loop trip is
// cut into the kernel's three steps, and any other wavefront may run between two of them:
//   ASK      feed_wants_grant -> the atomicAdd on the cursor (its value is kept aside, as the kernel keeps it in a register)
//   TAKE     some lanes are free: feed_pos for each of them, feed_advance
//   RECEIVE  feed_grant with the value the cursor had at ASK
// A wavefront makes its first request on its own before the loop, and leaves the loop when it holds no position and feed_finished says so.
// Built as a shared library for tests/test_match_feed_cpu.py, and with -DMATCHFEED_MAIN as a stand-alone program (a sanitizer build runs that).
// Never linked into libkallisto_amd.so.
#include "../../kallisto_amd/csrc/kamd_core.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {
struct Rng {   // splitmix64
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ULL); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; return z ^ (z >> 31); }
  uint32_t below(uint32_t m) { return (uint32_t)(next() % m); }
};
enum Step { ASK, TAKE, RECEIVE, DONE };
struct Wave { kamd::ItemFeed feed; Step step; bool asked; uint32_t granted; uint64_t trips; };
}  // namespace

// handed[p] (n + slack entries, zeroed by the caller) counts how often position p was given to a lane; *beyond: positions at or behind n that were
// handed out; *requests: atomicAdds made; *cursor_end: the cursor's final value.  Returns 0, or -1 if a wavefront did not finish within the trip limit.
extern "C" int emu_match_feed(uint32_t n, uint32_t grant, uint32_t n_waves, uint64_t seed, uint32_t* handed, uint64_t* beyond, uint64_t* requests,
                              uint64_t* cursor_end) {
  Rng rng{seed};
  uint64_t cursor = 0, n_beyond = 0, n_req = 0;
  std::vector<Wave> w(n_waves);
  // the wavefronts start in a random order: each makes its first request and looks at the answer at once
  std::vector<uint32_t> order(n_waves);
  for (uint32_t i = 0; i < n_waves; i++) order[i] = i;
  for (uint32_t i = n_waves; i > 1; i--) { const uint32_t j = rng.below(i); const uint32_t t = order[i - 1]; order[i - 1] = order[j]; order[j] = t; }
  for (uint32_t i : order) {
    w[i].feed = kamd::feed_open();
    const uint32_t start = (uint32_t)cursor; cursor += grant; ++n_req;
    kamd::feed_grant(w[i].feed, start, grant, n);
    w[i].step = ASK; w[i].asked = false; w[i].granted = 0; w[i].trips = 0;
  }
  uint32_t live = n_waves;
  const uint64_t trip_limit = 4ULL * n + 64;
  while (live) {
    Wave& v = w[rng.below(n_waves)];
    switch (v.step) {
      case ASK:
        v.asked = kamd::feed_wants_grant(v.feed);
        if (v.asked) { v.granted = (uint32_t)cursor; cursor += grant; ++n_req; }
        v.step = TAKE;
        break;
      case TAKE: {
        // 0 .. 64 free lanes (sometimes none, sometimes all: refill_min and the start of a wavefront)
        const uint32_t r = rng.below(8);
        const uint32_t want = r == 0 ? 0u : r == 1 ? 64u : 1u + rng.below(24);
        if (want && kamd::feed_avail(v.feed)) {
          for (uint32_t k = 0; k < want; k++) {
            uint32_t pos = 0;
            if (!kamd::feed_pos(v.feed, k, &pos)) continue;
            if (pos >= n) ++n_beyond; else ++handed[pos];
          }
          kamd::feed_advance(v.feed, want);
        }
        // the kernel's exit test sits here (no lane holds an item in this emulation once its position is counted)
        if (!v.asked && kamd::feed_finished(v.feed)) { v.step = DONE; --live; break; }
        v.step = RECEIVE;
        break;
      }
      case RECEIVE:
        if (v.asked) kamd::feed_grant(v.feed, v.granted, grant, n);
        v.step = ASK;
        if (++v.trips > trip_limit) return -1;
        break;
      case DONE:
        break;
    }
  }
  if (beyond) *beyond = n_beyond;
  if (requests) *requests = n_req;
  if (cursor_end) *cursor_end = cursor;
  return 0;
}

// the fixed-chunk form: wavefront w owns [w * items_per_wave, + items_per_wave) clipped to n, as k_match_v3 sets it up without a cursor
extern "C" int emu_match_feed_fixed(uint32_t n, uint32_t items_per_wave, uint64_t seed, uint32_t* handed, uint64_t* beyond) {
  Rng rng{seed};
  uint64_t n_beyond = 0;
  const uint64_t n_waves = ((uint64_t)n + items_per_wave - 1) / items_per_wave + 1;   // (one wavefront more than the grid would hold: its chunk is empty)
  for (uint64_t wv = 0; wv < n_waves; wv++) {
    const uint64_t c0 = wv * (uint64_t)items_per_wave, lo = c0 < n ? c0 : n, hi = c0 + items_per_wave < n ? c0 + items_per_wave : n;
    kamd::ItemFeed f = kamd::feed_fixed((uint32_t)lo, (uint32_t)hi);
    if (kamd::feed_wants_grant(f)) return -2;
    uint64_t trips = 0;
    while (!kamd::feed_finished(f)) {
      const uint32_t want = 1u + rng.below(64);
      for (uint32_t k = 0; k < want; k++) {
        uint32_t pos = 0;
        if (!kamd::feed_pos(f, k, &pos)) continue;
        if (pos >= n) ++n_beyond; else ++handed[pos];
      }
      kamd::feed_advance(f, want);
      if (kamd::feed_wants_grant(f)) return -2;
      if (++trips > (uint64_t)items_per_wave + 8) return -1;
    }
  }
  if (beyond) *beyond = n_beyond;
  return 0;
}

#ifdef MATCHFEED_MAIN
// the cases of tests/test_match_feed_cpu.py, self-checking: exit status 0 = every position of [0, n) exactly once, none beyond
int main() {
  const uint32_t grants[] = {64, 256, 1000}, waves[] = {1, 3, 24};
  int bad = 0, cases = 0;
  for (uint32_t g : grants) {
    const uint32_t ns[] = {0, 1, 63, 64, 65, g - 1, g, g + 1, 5000};
    for (uint32_t n : ns) for (uint32_t W : waves) for (uint64_t seed = 1; seed <= 4; seed++) {
      std::vector<uint32_t> handed(n + 1, 0);
      uint64_t beyond = 0, req = 0, end = 0;
      const int rc = emu_match_feed(n, g, W, seed * 7919 + n + g + W, handed.data(), &beyond, &req, &end);
      bool ok = rc == 0 && beyond == 0 && end == req * g;
      for (uint32_t p = 0; p < n; p++) ok = ok && handed[p] == 1;
      ++cases;
      if (!ok) { ++bad; std::fprintf(stderr, "FAIL n=%u grant=%u waves=%u seed=%llu rc=%d beyond=%llu\n", n, g, W, (unsigned long long)seed, rc, (unsigned long long)beyond); }
    }
    for (uint32_t n : ns) {
      std::vector<uint32_t> handed(n + 1, 0);
      uint64_t beyond = 0;
      const int rc = emu_match_feed_fixed(n, g, n + g, handed.data(), &beyond);
      bool ok = rc == 0 && beyond == 0;
      for (uint32_t p = 0; p < n; p++) ok = ok && handed[p] == 1;
      ++cases;
      if (!ok) { ++bad; std::fprintf(stderr, "FAIL fixed n=%u items_per_wave=%u rc=%d\n", n, g, rc); }
    }
  }
  std::printf("%d cases, %d failed\n", cases, bad);
  return bad ? 1 : 0;
}
#endif
