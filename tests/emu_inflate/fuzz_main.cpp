// tests/emu_inflate/fuzz_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program (built with -fsanitize=address,undefined by `make fuzz`)
// that feeds kamd_inflate.h's decoder the streams of a directory, as tests/inflate_streams.py writes them:
//   <name>.valid / <name>.bad   u32 isize, u32 crc32, then the raw deflate stream (exactly as long as the member says: the sanitizer sees
//                               every read behind it)
//   <name>.out                  the text a .valid stream must give
// Exit 0: every valid stream decodes to its text, every damaged one is refused, and the sanitizers had nothing to say.
#include "../../kallisto_amd/csrc/kamd_inflate.h"

#include <dirent.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace kamd::inf;

static bool slurp(const std::string& p, std::vector<uint8_t>* v) {
  FILE* f = fopen(p.c_str(), "rb");
  if (!f) return false;
  v->clear();
  uint8_t buf[65536]; size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v->insert(v->end(), buf, buf + n);
  fclose(f);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <directory of streams>\n", argv[0]); return 2; }
  DIR* d = opendir(argv[1]);
  if (!d) { perror(argv[1]); return 2; }
  int n_valid = 0, n_bad = 0, failures = 0;
  Work* w = new Work;
  while (dirent* e = readdir(d)) {
    const std::string name = e->d_name;
    const bool valid = name.size() > 6 && name.compare(name.size() - 6, 6, ".valid") == 0;
    const bool bad = name.size() > 4 && name.compare(name.size() - 4, 4, ".bad") == 0;
    if (!valid && !bad) continue;
    std::vector<uint8_t> file, want;
    if (!slurp(std::string(argv[1]) + "/" + name, &file) || file.size() < 8) { fprintf(stderr, "%s: unreadable\n", name.c_str()); ++failures; continue; }
    uint32_t isize, crc;
    memcpy(&isize, file.data(), 4); memcpy(&crc, file.data() + 4, 4);
    if (isize > MAX_ISIZE) { fprintf(stderr, "%s: ISIZE beyond a member\n", name.c_str()); ++failures; continue; }
    // exact-size heap copies: a read or write one byte outside either is a sanitizer report
    std::vector<uint8_t> src(file.begin() + 8, file.end()), out(isize);
    int r = inflate_member(src.data(), (uint32_t)src.size(), out.data(), isize, *w, 0, 1, [] {});
    if (!r) {
      crc_table_fill(w->crc_tab, 0, 1);
      uint32_t nl = 0;
      if (~crc_slice_term(out.data(), isize, w->crc_tab, 0, 1, &nl) != crc) r = INF_CRC;
    }
    if (valid) {
      ++n_valid;
      if (!slurp(std::string(argv[1]) + "/" + name.substr(0, name.size() - 6) + ".out", &want)) { fprintf(stderr, "%s: no .out\n", name.c_str()); ++failures; continue; }
      if (r || want != out) { fprintf(stderr, "%s: valid stream %s (reason %d)\n", name.c_str(), r ? "refused" : "decoded to other bytes", r); ++failures; }
    } else {
      ++n_bad;
      if (!r) { fprintf(stderr, "%s: damaged stream accepted\n", name.c_str()); ++failures; }
    }
  }
  closedir(d);
  delete w;
  printf("%d valid, %d damaged, %d failures\n", n_valid, n_bad, failures);
  return failures || !n_valid || !n_bad ? 1 : 0;
}
