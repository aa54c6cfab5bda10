// kamd_inflate_feed.h -- `--inflate device`: BGZF FASTQ whose text never exists on the host.
//
// The host walks the member headers of the file(s) (as TextSource's constructor does) and, unit by unit, copies the raw DEFLATE streams of
// a run of whole members into pinned memory and from there to the device; kamd_bgzf_inflate decodes them behind the incomplete tail the
// previous unit left at the head of the text buffer, kamd_text_cut finds the whole records at the head of the text(s) (the same count in
// both mates' files), kamd_fastq_unit_parse takes them, and what lies behind the cut is copied device-to-device to the head of the next
// buffer.  Units reach `run` in input order, batched like UnitFeeder's.  One context; one unit at a time (the calls are synchronous: the
// next unit's compressed bytes are not staged while the device works on this one).
//
// A file takes members until tail + new text reaches the target, so a file whose tail is long takes fewer: the mates' tails drift, but
// stay below one unit.  Errors are the host path's: `<file>: corrupt BGZF block <i>`, "paired-end files have different numbers of reads";
// text that is not strict 4-line FASTQ is DECLINED and the caller starts over with the general reader.
#pragma once
#include "kamd_frontend.h"

namespace kamd_fe {

class InflateFeeder {
 public:
  enum { OK = UnitFeeder::OK, FAILED = UnitFeeder::FAILED, DECLINED = UnitFeeder::DECLINED };
  InflateFeeder(kamd_ctx* ctx, int device, std::function<int(int, PackedBatch&, std::string&)> run, UnitFeeder::Sizes z = UnitFeeder::sizes_from_env())
      : ctx_(ctx), dev_(device), run_(std::move(run)), z_(z) {
    cap_ = z_.max_unit + (1u << 16);   // a unit may overshoot its target by one member
  }
  ~InflateFeeder() {
    (void)hipSetDevice(dev_);
    for (auto& b : bufs_) for (int f = 0; f < 2; f++) if (b.d[f]) (void)hipFree(b.d[f]);
    for (int f = 0; f < 2; f++) { if (pin_[f]) (void)hipHostFree(pin_[f]); if (d_comp_[f]) (void)hipFree(d_comp_[f]); }
    if (copy_) (void)hipStreamDestroy(copy_);
  }
  static bool all_bgzf(const std::vector<std::string>& files, std::string* first_other) {
    for (const auto& f : files) if (!BgzfSource::is_bgzf(f)) { *first_other = f; return false; }
    return true;
  }
  const std::string& error() const { return error_; }
  uint64_t units = 0, comp_bytes = 0, text_bytes = 0;
  double stage_s = 0.0, inflate_s = 0.0, cut_s = 0.0, parse_s = 0.0, run_s = 0.0;

  int feed(const std::string& f0, const std::string* f1, uint64_t& n_items, bool verbose) {
    const int nf = f1 ? 2 : 1;
    File file[2];
    for (int f = 0; f < nf; f++) if (!file[f].open(f ? *f1 : f0, &error_)) return FAILED;
    if (prepare(nf) != OK) return FAILED;
    uint64_t tail[2] = {0, 0}, lines_in[2] = {0, 0}, records = 0;
    std::vector<int> pending;
    uint64_t pending_records = 0;
    int cur = take_buffer(-1);
    int rc = OK;
    auto flush = [&]() -> int {
      if (pending.empty()) return OK;
      const auto t0 = now();
      kamd_fastq_unit fu;
      if (kamd_fastq_batch_pack(ctx_, &fu) != 0) { error_ = kamd_last_error(); return FAILED; }
      if (fu.n_items) {
        PackedBatch pb;
        pb.d_words = const_cast<uint32_t*>(fu.d_words); pb.d_len = const_cast<uint16_t*>(fu.d_len);
        pb.n_items = fu.n_items; pb.n_reads = fu.n_items * (uint64_t)nf; pb.max_len = fu.max_len; pb.filled = true;
        std::string err;
        if (run_(0, pb, err)) { error_ = err; return FAILED; }
      }
      run_s += since(t0);
      for (int bi : pending) bufs_[bi].busy = false;
      pending.clear(); pending_records = 0;
      return OK;
    };
    for (;;) {
      Buf& b = bufs_[cur];
      bool all_done = true, took = false;
      // ---- the next run of whole members of every file, inflated behind the tail ----
      for (int f = 0; f < nf && rc == OK; f++) {
        File& F = file[f];
        const size_t first = F.next;
        uint64_t text = 0, comp = 0;
        members_.clear();
        while (F.next < F.members.size()) {
          const Member& m = F.members[F.next];
          if (tail[f] + text + m.isize > z_.max_unit || comp + m.src_len > comp_cap_) break;
          if (text && tail[f] + text >= z_.target) break;
          members_.push_back(kamd_bgzf_member{comp, m.src_len, m.isize, m.crc, 0u, tail[f] + text});
          text += m.isize; comp += m.src_len; ++F.next;
        }
        if (F.next > first) {
          took = true;
          auto t0 = now();
          uint64_t at = 0;
          for (size_t i = first; i < F.next; i++) { memcpy(pin_[f] + at, F.map + F.members[i].src_off, F.members[i].src_len); at += F.members[i].src_len; }
          if (hipMemcpyAsync(d_comp_[f], pin_[f], comp, hipMemcpyHostToDevice, copy_) != hipSuccess || hipStreamSynchronize(copy_) != hipSuccess) {
            error_ = "copy of compressed bytes to the device failed"; rc = FAILED; break;
          }
          stage_s += since(t0); t0 = now();
          kamd_inflate_result res;
          if (kamd_bgzf_inflate(ctx_, (const uint8_t*)d_comp_[f], comp, members_.data(), members_.size(), b.d[f], cap_, &res) != 0) { error_ = kamd_last_error(); rc = FAILED; break; }
          inflate_s += since(t0);
          if (res.status != 0) { error_ = F.path + ": corrupt BGZF block " + std::to_string(first + res.first_bad_member); rc = FAILED; break; }
          tail[f] += text; lines_in[f] += res.n_newlines;
          comp_bytes += comp; text_bytes += text;
        }
        if (F.next == F.members.size() && !F.closed) {   // the end of the text: a final newline is appended where it lacks
          F.closed = true;
          char last = '\n';
          if (tail[f] && (hipMemcpyAsync(&last, b.d[f] + tail[f] - 1, 1, hipMemcpyDeviceToHost, copy_) != hipSuccess || hipStreamSynchronize(copy_) != hipSuccess)) {
            error_ = "read-back of the text's last byte failed"; rc = FAILED; break;
          }
          if (last != '\n') {
            if (hipMemcpyAsync(b.d[f] + tail[f], "\n", 1, hipMemcpyHostToDevice, copy_) != hipSuccess || hipStreamSynchronize(copy_) != hipSuccess) {
              error_ = "copy to the device failed"; rc = FAILED; break;
            }
            ++tail[f]; ++lines_in[f];
          }
        }
        all_done = all_done && F.next == F.members.size();
      }
      if (rc != OK) break;
      // ---- whole records at the head of the text(s) ----
      uint64_t R = 0, end[2] = {0, 0};
      bool any_text = false;
      for (int f = 0; f < nf; f++) any_text = any_text || tail[f];
      if (any_text) {
        const auto t0 = now();
        const char* txt[2] = {b.d[0], b.d[1]};
        if (kamd_text_cut(ctx_, txt, tail, nf, ~0ull, &R, end) != 0) { error_ = kamd_last_error(); rc = FAILED; break; }
        cut_s += since(t0);
      }
      uint64_t left_lines[2] = {0, 0};
      for (int f = 0; f < nf; f++) left_lines[f] = lines_in[f] - 4 * (records + R);
      if (R) {
        const auto t0 = now();
        kamd_fastq_unit fu;
        const char* txt[2] = {b.d[0], b.d[1]};
        if (kamd_fastq_unit_parse(ctx_, txt, end, nf, R, &fu) != 0) { error_ = kamd_last_error(); rc = FAILED; break; }
        parse_s += since(t0);
        if (fu.status == 3) { error_ = "reads longer than 65535 bp are outside the short-read GPU path"; rc = FAILED; break; }
        pending.push_back(cur);   // (the text stays in place until the batch is packed)
        if (fu.status != 0) { rc = DECLINED; break; }
        records += R; pending_records += R; n_items += R; ++units;
        if (verbose) std::cerr << "[quant] processed " << n_items << (nf == 2 ? " pairs" : " reads") << std::endl;
        // what lies behind the cut goes to the head of the next buffer
        int nb = take_buffer(cur);
        if (nb < 0) { if ((rc = flush()) != OK) break; nb = take_buffer(cur); }   // (packed: the buffers of the batch are free, this one's bytes still lie there)
        bool ok = true;
        for (int f = 0; f < nf && ok; f++) {
          const uint64_t n = tail[f] - end[f];
          if (n) ok = hipMemcpyAsync(bufs_[nb].d[f], b.d[f] + end[f], n, hipMemcpyDeviceToDevice, copy_) == hipSuccess;
          tail[f] = n;
        }
        if (!ok || hipStreamSynchronize(copy_) != hipSuccess) { error_ = "device-to-device copy of a unit's tail failed"; rc = FAILED; break; }
        cur = nb;
        if (pending_records >= z_.batch_items || pending.size() + 2 >= bufs_.size()) { if ((rc = flush()) != OK) break; }
      }
      // ---- a file has ended short of the other: the mates' files hold different numbers of records ----
      bool mismatch = false;
      for (int f = 0; f < nf; f++) {
        const int o = nf - 1 - f;
        if (nf == 2 && file[f].closed && left_lines[f] < 4 && left_lines[o] >= 4) mismatch = true;
      }
      if (mismatch) { error_ = "paired-end files have different numbers of reads"; rc = FAILED; break; }
      if (all_done) {
        // what remains must be blank; lines that are no whole record leave the decision to the general reader
        for (int f = 0; f < nf && rc == OK; f++) {
          if (!tail[f]) continue;
          std::vector<char> rest(tail[f]);
          if (hipMemcpyAsync(rest.data(), bufs_[cur].d[f], tail[f], hipMemcpyDeviceToHost, copy_) != hipSuccess || hipStreamSynchronize(copy_) != hipSuccess) { error_ = "read-back of the text's end failed"; rc = FAILED; break; }
          for (char c : rest) if (c != '\n' && c != '\r' && c != ' ' && c != '\t') { rc = DECLINED; break; }
        }
        break;
      }
      if (!took && !R) { rc = DECLINED; break; }   // a record that no buffer holds: not what this path is for
    }
    if (rc == OK) rc = flush();
    else if (!pending.empty()) { kamd_fastq_unit fu; (void)kamd_fastq_batch_pack(ctx_, &fu); }   // (the units parsed so far leave the context's batch)
    for (auto& b : bufs_) b.busy = false;
    return rc;
  }

 private:
  struct Member { uint64_t src_off; uint32_t src_len, isize, crc; };
  struct File {
    std::string path; int fd = -1; const unsigned char* map = nullptr; uint64_t size = 0;
    std::vector<Member> members; size_t next = 0; bool closed = false;
    // the members with text, hopping from header to header (the empty ones -- the EOF marker, also between concatenated files -- are skipped)
    bool open(const std::string& p, std::string* err) {
      path = p;
      fd = ::open(p.c_str(), O_RDONLY);
      struct stat st;
      if (fd < 0 || fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { *err = "could not open " + p + " as a regular file"; return false; }
      size = (uint64_t)st.st_size;
      if (!size) return true;
      void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
      if (m == MAP_FAILED) { *err = "could not map " + p; return false; }
      map = (const unsigned char*)m;
      (void)madvise(m, size, MADV_SEQUENTIAL);
      for (uint64_t o = 0; o < size;) {
        size_t bs = 0, doff = 0;
        if (!BgzfSource::header(map + o, size - o, &bs, &doff) || o + bs > size || bs < doff + 8) { *err = p + ": broken BGZF block at offset " + std::to_string(o); return false; }
        const unsigned char* t = map + o + bs - 8;
        const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        const uint32_t isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
        if (isize > 65536) { *err = p + ": broken BGZF block at offset " + std::to_string(o); return false; }
        if (isize) members.push_back(Member{o + doff, (uint32_t)(bs - doff - 8), isize, crc});
        o += bs;
      }
      return true;
    }
    ~File() { if (map) munmap((void*)map, size); if (fd >= 0) ::close(fd); }
  };
  struct Buf { char* d[2] = {nullptr, nullptr}; bool busy = false; };
  static std::chrono::steady_clock::time_point now() { return std::chrono::steady_clock::now(); }
  static double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(now() - t0).count(); }
  // a text buffer that is neither the current one nor part of the batch under construction, now taken; -1: none
  int take_buffer(int not_this) {
    for (size_t i = 0; i < bufs_.size(); i++) if (!bufs_[i].busy && (int)i != not_this) { bufs_[i].busy = true; return (int)i; }
    return -1;
  }
  int prepare(int nf) {
    if (hipSetDevice(dev_) != hipSuccess) { error_ = "hipSetDevice failed"; return FAILED; }
    if (!copy_ && hipStreamCreateWithFlags(&copy_, hipStreamNonBlocking) != hipSuccess) { error_ = "hipStreamCreate failed"; return FAILED; }
    if (bufs_.empty()) bufs_.resize((size_t)std::max(4, z_.bufs));
    comp_cap_ = z_.max_unit;   // (a member's stream is rarely longer than its text; a unit stops where its compressed bytes would not fit)
    for (int f = 0; f < nf; f++) {
      if (!pin_[f] && hipHostMalloc((void**)&pin_[f], comp_cap_, hipHostMallocDefault) != hipSuccess) { error_ = "pinned allocation of the compressed staging buffer failed"; return FAILED; }
      if (!d_comp_[f] && hipMalloc((void**)&d_comp_[f], comp_cap_ + 64) != hipSuccess) { error_ = "device allocation of the compressed buffer failed"; return FAILED; }
      for (auto& b : bufs_) if (!b.d[f] && hipMalloc((void**)&b.d[f], cap_ + 64) != hipSuccess) { error_ = "device allocation of a text buffer failed"; return FAILED; }
    }
    return OK;
  }
  kamd_ctx* ctx_; int dev_;
  std::function<int(int, PackedBatch&, std::string&)> run_;
  UnitFeeder::Sizes z_;
  size_t cap_ = 0, comp_cap_ = 0;
  std::vector<Buf> bufs_;
  char* pin_[2] = {nullptr, nullptr}; char* d_comp_[2] = {nullptr, nullptr};
  hipStream_t copy_ = nullptr;
  std::vector<kamd_bgzf_member> members_;
  std::string error_;
};

// feed_files with `--inflate device`: `inflater` null = --inflate host (today's path, untouched).  Input the device path does not take
// (a file that is not BGZF; `one_context` false: several GPUs, --share-device) is said in one line and goes down the host path.
inline int feed_files_inflate(const std::vector<std::string>& files, bool paired, uint64_t batch, int host_threads, int io_threads, bool verbose,
                              MultiPipe& pipe, uint64_t& n_processed, double& pack_s, UnitFeeder* units, const std::function<int()>& reset,
                              InflateFeeder* inflater, bool one_context) {
  if (!inflater) return feed_files(files, paired, batch, host_threads, io_threads, verbose, pipe, n_processed, pack_s, units, reset);
  std::string other = files.empty() ? std::string("the input") : files[0];
  if (!one_context || !InflateFeeder::all_bgzf(files, &other)) {
    // (one write: the index thread prints its lines meanwhile, and pieces of two lines may otherwise alternate)
    std::cerr << std::string("[quant] --inflate device: " + other + " is not BGZF (or the run uses several contexts); inflating on the host\n") << std::flush;
    return feed_files(files, paired, batch, host_threads, io_threads, verbose, pipe, n_processed, pack_s, units, reset);
  }
  const uint64_t n_before = n_processed;
  if (verbose) std::cerr << std::string("[quant] BGZF input is inflated on the device\n") << std::flush;
  int rc = InflateFeeder::OK;
  for (size_t fi = 0; fi < files.size() && rc == InflateFeeder::OK; fi += paired ? 2 : 1)
    rc = inflater->feed(files[fi], paired ? &files[fi + 1] : nullptr, n_processed, verbose);
  if (rc == InflateFeeder::OK) {
    if (verbose) std::cerr << "[timing] device inflate: " << inflater->units << " units, " << inflater->comp_bytes / 1000000 << " MB compressed -> " << inflater->text_bytes / 1000000
                           << " MB of text; staging " << inflater->stage_s << " s, inflate " << inflater->inflate_s << " s, cut " << inflater->cut_s << " s, parse "
                           << inflater->parse_s << " s, pack + pseudoalign " << inflater->run_s << " s" << std::endl;
    return 0;
  }
  if (rc == InflateFeeder::FAILED) { std::cerr << "Error: " << inflater->error() << std::endl; return 1; }
  // declined: not (only) strict 4-line FASTQ -- start over with the general reader, exactly as after UnitFeeder::DECLINED
  if (verbose) std::cerr << "[quant] input is not strict 4-line FASTQ: reading it with the general FASTA/FASTQ reader" << std::endl;
  if (reset && reset()) { std::cerr << "Error: " << kamd_last_error() << std::endl; return 1; }
  n_processed = n_before;
  return feed_files(files, paired, batch, host_threads, io_threads, verbose, pipe, n_processed, pack_s, nullptr, reset);
}

}  // namespace kamd_fe
