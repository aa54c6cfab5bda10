// kamd_bus.cpp -- host side of the barcode / UMI technologies: technology name or "bc:umi:seq" string -> kamd_bus_layout (kamd_bus_layout_parse),
// the check of a layout (kamd::bus_layout_check), kamd_bus_seq_max_len, and the text of a barcode whitelist -> codes (kamd_bus_whitelist_parse).  No GPU code, no dependency on the rest of the library: tests/emu_bustag
// compiles this file for the CPU as it is.
//
// The reference keeps one branch per technology name (src/main.cpp:1283-1408) and a parser for custom strings (ParseTechnology, :778-870).  Here a name is
// an alias of the custom string that describes the same layout, so there is one parser; the table below restates the reference's values in that form.
#include "kamd_bustag.h"

#include <cctype>
#include <cerrno>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

enum { STRAND_NONE = 0, STRAND_FR = 1 };

struct Alias { const char* name; const char* layout; int strand; };
// file,start,stop triples: barcode parts : UMI parts : sequence part
const Alias ALIASES[] = {
    {"10XV2", "0,0,16:0,16,26:1,0,0", STRAND_FR},
    {"10XV3", "0,0,16:0,16,28:1,0,0", STRAND_FR},
    {"VISIUM", "0,0,16:0,16,28:1,0,0", STRAND_FR},
    {"SURECELL", "0,0,6,0,21,27,0,42,48:0,51,59:1,0,0", STRAND_FR},
    {"DROPSEQ", "0,0,12:0,12,20:1,0,0", STRAND_NONE},
    {"INDROPSV1", "0,0,11,0,30,38:0,42,48:1,0,0", STRAND_NONE},
    {"INDROPSV2", "1,0,11,1,30,38:1,42,48:0,0,0", STRAND_NONE},
    {"CELSEQ", "0,0,8:0,8,12:1,0,0", STRAND_FR},
    {"CELSEQ2", "0,6,12:0,0,6:1,0,0", STRAND_FR},
    {"SPLIT-SEQ", "1,10,18,1,48,56,1,78,86:1,0,10:0,0,0", STRAND_FR},
    {"SCRBSEQ", "0,0,6:0,6,16:1,0,0", STRAND_NONE},
    {"BDWTA", "0,0,9,0,21,30,0,43,52:0,52,60:1,0,0", STRAND_FR},   // the three cell-label sections between their linkers, then the UMI
    {"VASA-SEQ", "0,6,14:0,0,6:0,14,0", STRAND_FR},
};
struct Refusal { const char* name; const char* why; };
const Refusal REFUSED[] = {
    {"10XV1", "reads three files per read set; a layout here has one or two"},
    {"INDROPSV3", "reads three files per read set; a layout here has one or two"},
    {"SMARTSEQ2", "reads three or four files per read set; a layout here has one or two"},
    {"SMARTSEQ3", "reads four files per read set, has two sequence parts and a tag sequence"},
    {"STORM-SEQ", "has two sequence parts (paired-end reads); a layout here has exactly one"},
    {"BULK", "is not a barcode / UMI technology: whole reads go to kamd_pseudoalign as they are"},
};

int set_err(char* err, size_t cap, const std::string& msg) {
  if (err && cap) { snprintf(err, cap, "%s", msg.c_str()); }
  return -1;
}

std::string upper(const std::string& s) {
  std::string r = s;
  for (char& c : r) c = (char)toupper((unsigned char)c);
  return r;
}

// std::stoi's reading of a token: leading white space, an optional sign, digits; what follows the digits is ignored.  0 ok, 1 no number, 2 out of range
int to_int(const std::string& t, int* out) {
  const char* s = t.c_str();
  char* end = nullptr;
  errno = 0;
  const long v = strtol(s, &end, 10);
  if (end == s) return 1;
  if (errno == ERANGE || v < INT_MIN || v > INT_MAX) return 2;
  *out = (int)v;
  return 0;
}

// one of the three lists.  The messages are ParseTechnology's.
bool parse_list(const std::string& s, std::vector<kamd_bus_substr>& v, int& max_file, std::string& why) {
  std::vector<int> vals;
  v.clear();
  for (size_t pos = 0; pos < s.size();) {   // tokens as std::getline(ss, t, ',') cuts them: "a,b," has two, "," has one empty one
    size_t comma = s.find(',', pos);
    if (comma == std::string::npos) comma = s.size();
    const std::string t = s.substr(pos, comma - pos);
    int x = 0;
    const int rc = to_int(t, &x);
    if (rc == 1) { why = "Error: converting to int: \"" + t + "\""; return false; }
    if (rc == 2) { why = "Error: value out of range: \"" + t + "\""; return false; }   // (the reference lets std::out_of_range escape)
    vals.push_back(x);
    pos = comma + 1;
  }
  if (vals.size() % 3 != 0) { why = "Error: number of values has to be multiple of 3 " + s; return false; }
  for (size_t i = 0; i + 2 < vals.size(); i += 3) {
    const int f = vals[i], a = vals[i + 1], b = vals[i + 2];
    if (f < -1) { why = "Error: invalid file number (" + std::to_string(f) + ")  " + s; return false; }
    if (a < 0 && f != -1) { why = "Error: invalid start (" + std::to_string(a) + ")  " + s; return false; }
    if (b != 0 && b <= a && f != -1) {
      why = "Error: invalid stop (" + std::to_string(b) + ") has to be after start (" + std::to_string(a) + ")  " + s;
      return false;
    }
    v.push_back(kamd_bus_substr{f, a, b});
    if (f > max_file) max_file = f;
  }
  return true;
}

bool parse_custom(const std::string& tech, kamd_bus_layout* L, std::string& why) {
  const size_t i1 = tech.find(':');
  const char* head = "Error: technology string must contain two colons (:), ";
  if (i1 == std::string::npos) { why = std::string(head) + "none found: \"" + tech + "\""; return false; }
  const size_t i2 = tech.find(':', i1 + 1);
  if (i2 == std::string::npos) { why = std::string(head) + "only one found: \"" + tech + "\""; return false; }
  if (tech.find(':', i2 + 1) != std::string::npos) { why = std::string(head) + "three found: \"" + tech + "\""; return false; }
  const std::string bcs = tech.substr(0, i1), umis = tech.substr(i1 + 1, i2 - i1 - 1), seqs = tech.substr(i2 + 1);
  std::vector<kamd_bus_substr> bc, umi, seq;
  int max_file = 0;
  if (!parse_list(bcs, bc, max_file, why)) return false;
  if (bc.empty()) { why = "Error: empty barcode list " + bcs; return false; }
  if (umis == "RX") { why = "a UMI in the FASTQ comment (RX) is not supported: the packed reads carry no comments"; return false; }
  if (!parse_list(umis, umi, max_file, why)) return false;
  if (umi.empty()) { why = "Error: empty UMI list " + umis; return false; }
  if (!parse_list(seqs, seq, max_file, why)) return false;
  if (seq.empty()) { why = "Error: empty sequence list " + bcs; return false; }   // (the reference prints the barcode list here)
  // what this library takes of it
  if (seq.size() != 1) { why = "a layout has exactly one sequence part, this one has " + std::to_string(seq.size()) + " (paired-end technologies are not supported)"; return false; }
  if (bc.size() > KAMD_BUS_MAX_PARTS || umi.size() > KAMD_BUS_MAX_PARTS) {
    why = "a field has at most " + std::to_string(KAMD_BUS_MAX_PARTS) + " parts";
    return false;
  }
  memset(L, 0, sizeof *L);
  L->n_files = max_file + 1;
  L->n_bc = (int32_t)bc.size();
  L->n_umi = (int32_t)umi.size();
  for (size_t i = 0; i < bc.size(); i++) L->bc[i] = bc[i];
  for (size_t i = 0; i < umi.size(); i++) L->umi[i] = umi[i];
  L->seq = seq[0];
  char buf[256];
  if (kamd::bus_layout_check(L, buf, sizeof buf)) { why = buf; return false; }
  return true;
}

// false: the field is not one kamd_bus_split takes, `why` says which rule it breaks
bool field_ok(const kamd_bus_substr* p, int n, int n_files, const char* what, std::string& why) {
  if (n < 1 || n > KAMD_BUS_MAX_PARTS) { why = std::string(what) + ": 1 to " + std::to_string(KAMD_BUS_MAX_PARTS) + " parts"; return false; }
  if (p[0].file == -1) {
    if (n != 1) { why = std::string(what) + ": file -1 (the field is absent) stands alone"; return false; }
    return true;
  }
  long fixed = 0;
  bool all_fixed = true;
  for (int i = 0; i < n; i++) {
    if (p[i].file < 0 || p[i].file >= n_files) { why = std::string(what) + ": part " + std::to_string(i) + " names file " + std::to_string(p[i].file) + " of " + std::to_string(n_files); return false; }
    if (p[i].start < 0 || p[i].start > 65535 || p[i].stop < 0 || p[i].stop > 65535) { why = std::string(what) + ": start and stop lie in [0, 65535] (the longest packed read)"; return false; }
    if (p[i].stop != 0 && p[i].stop <= p[i].start) { why = std::string(what) + ": stop has to be 0 or after start"; return false; }
    if (p[i].stop == 0) all_fixed = false; else fixed += p[i].stop - p[i].start;
  }
  if (all_fixed && fixed > 32) {
    why = std::string(what) + ": " + std::to_string(fixed) + " fixed bases, a BUS field holds 32 (the reference truncates; refused here)";
    return false;
  }
  return true;
}

}  // namespace

namespace kamd {
int bus_layout_check(const kamd_bus_layout* L, char* err, size_t err_cap) {
  if (!L) return set_err(err, err_cap, "null layout");
  std::string why;
  if (L->n_files < 1 || L->n_files > 2)
    return set_err(err, err_cap, "a layout reads one or two files per read set, this one " + std::to_string(L->n_files));
  if (!field_ok(L->bc, L->n_bc, L->n_files, "barcode", why) || !field_ok(L->umi, L->n_umi, L->n_files, "UMI", why)) return set_err(err, err_cap, why);
  if (L->seq.file < 0 || L->seq.file >= L->n_files) return set_err(err, err_cap, "sequence: names file " + std::to_string(L->seq.file) + " of " + std::to_string(L->n_files));
  if (L->seq.start < 0 || L->seq.start > 65535 || L->seq.stop < 0 || L->seq.stop > 65535) return set_err(err, err_cap, "sequence: start and stop lie in [0, 65535] (the longest packed read)");
  if (L->seq.stop != 0 && L->seq.stop <= L->seq.start) return set_err(err, err_cap, "sequence: stop has to be 0 or after start");
  return 0;
}
}  // namespace kamd

extern "C" int kamd_bus_layout_parse(const char* technology, kamd_bus_layout* out, int32_t* default_strand, char* err, size_t err_cap) {
  if (err && err_cap) err[0] = 0;
  if (!technology || !out) return set_err(err, err_cap, "kamd_bus_layout_parse: null argument");
  const std::string tech(technology), up = upper(tech);
  for (const Refusal& r : REFUSED)
    if (up == r.name) return set_err(err, err_cap, "technology " + up + " " + r.why);
  std::string why;
  int strand = STRAND_NONE;
  const char* text = nullptr;
  for (const Alias& a : ALIASES)
    if (up == a.name) { text = a.layout; strand = a.strand; }
  kamd_bus_layout L;
  if (!parse_custom(text ? std::string(text) : tech, &L, why)) return set_err(err, err_cap, why);
  *out = L;
  if (default_strand) *default_strand = strand;
  return 0;
}

extern "C" int32_t kamd_bus_seq_max_len(const kamd_bus_layout* L, int32_t max_len) {
  if (!L || max_len <= 0) return 1;
  const int32_t end = (L->seq.stop && L->seq.stop < max_len) ? L->seq.stop : max_len;
  const int32_t n = end - L->seq.start;
  return n > 1 ? n : 1;
}

// ---- barcode whitelists: the text of a whitelist file -> codes (kamd_bus_whitelist_parse).  The caller reads the file; lines are counted from 1,
// empty ones included, so that an error names the line an editor shows ----
extern "C" int kamd_bus_whitelist_parse(const char* text, size_t len, uint64_t* out, uint64_t cap, uint64_t* n, int32_t* bc_len, char* err, size_t err_cap) {
  if (err && err_cap) err[0] = 0;
  if (n) *n = 0;
  if (bc_len) *bc_len = 0;
  if ((!text && len) || !n || !bc_len) return set_err(err, err_cap, "kamd_bus_whitelist_parse: null argument");
  uint64_t count = 0, line = 0;
  size_t L = 0;
  for (size_t pos = 0; pos < len;) {
    size_t end = pos;
    while (end < len && text[end] != '\n') ++end;
    size_t stop = end;
    if (stop > pos && text[stop - 1] == '\r') --stop;
    ++line;
    const size_t l = stop - pos;
    if (l) {
      if (l > 32) return set_err(err, err_cap, "whitelist line " + std::to_string(line) + ": " + std::to_string(l) + " bases, a barcode holds at most 32");
      if (count == 0) L = l;
      else if (l != L)
        return set_err(err, err_cap, "whitelist line " + std::to_string(line) + ": " + std::to_string(l) + " bases, the first barcode has " + std::to_string(L));
      uint64_t code = 0;
      for (size_t i = pos; i < stop; i++) {
        int b;
        switch (text[i]) {
          case 'A': case 'a': b = 0; break;
          case 'C': case 'c': b = 1; break;
          case 'G': case 'g': b = 2; break;
          case 'T': case 't': b = 3; break;
          default: {
            char shown[8];
            const unsigned char ch = (unsigned char)text[i];
            if (ch >= 0x21 && ch < 0x7F) snprintf(shown, sizeof shown, "'%c'", (char)ch); else snprintf(shown, sizeof shown, "0x%02X", ch);
            return set_err(err, err_cap, "whitelist line " + std::to_string(line) + ": " + shown + " at base " + std::to_string(i - pos + 1) + " is not one of ACGT");
          }
        }
        code = (code << 2) | (uint64_t)b;
      }
      if (out && count < cap) out[count] = code;
      ++count;
    }
    pos = end + 1;
  }
  *n = count;
  *bc_len = (int32_t)L;
  if (count == 0) return set_err(err, err_cap, "whitelist: no barcode in it");
  if (out && count > cap) return set_err(err, err_cap, "whitelist: " + std::to_string(count) + " barcodes, the output holds " + std::to_string(cap));
  return 0;
}
