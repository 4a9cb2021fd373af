// device_reader.cc — see device_reader.h.
#include "device_reader.h"

#include <algorithm>
#include <chrono>
#include <cstring>

#include "gpu_adapters.h"

namespace difacto {

static double Seconds() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

DeviceTextFeed::DeviceTextFeed(dfx_ctx* ctx, size_t batch_size, size_t shuf_buf,
                               const std::string& format, int nslots, int nring)
    : batch_size_(batch_size ? batch_size : 1),
      shuf_buf_(shuf_buf),
      format_(format == "libsvm"  ? DFX_TEXT_LIBSVM
              : format == "adfea" ? DFX_TEXT_ADFEA
                                  : DFX_TEXT_CRITEO) {
  DfxCheck(dfx_textfeed_create(ctx, nslots, nring, (int64_t)batch_size_, (int64_t)shuf_buf_,
                               format_, &h_),
           "dfx_textfeed_create");
  slot_held_.assign((size_t)nslots, false);
  ring_out_.assign((size_t)nring, false);
}

DeviceTextFeed::~DeviceTextFeed() {
  if (h_) dfx_textfeed_destroy(h_);
}

void DeviceTextFeed::BeginBatch() {
  int cur = -1;
  DfxCheck(dfx_textfeed_counts(h_, nullptr, nullptr, &cur), "dfx_textfeed_counts");
  const int next = (cur + 1) % nring();
  if (ring_out_[next])
    throw FeedProtocolError(
        "text feed: the ring came round to a batch that was handed out and never marked (a "
        "missing Consumed / Mark, or a ring no deeper than the caller's deferral)");
  DfxCheck(dfx_textfeed_batch_begin(h_), "dfx_textfeed_batch_begin");
}

void DeviceTextFeed::HandOutEntry() {
  int cur = -1;
  DfxCheck(dfx_textfeed_counts(h_, nullptr, nullptr, &cur), "dfx_textfeed_counts");
  if (cur < 0) throw FeedProtocolError("text feed: no batch begun");
  ring_out_[cur] = true;
  out_.push_back(Out{next_ticket_++, false, cur});
}

void DeviceTextFeed::HandOutSlot(int slot) {
  if (slot < 0 || slot >= nslots() || slot_held_[slot])
    throw FeedProtocolError("text feed: a slot handed out twice");
  slot_held_[slot] = true;
  out_.push_back(Out{next_ticket_++, true, slot});
}

int DeviceTextFeed::SlotsHeld() const {
  int n = 0;
  for (bool b : slot_held_) n += b;
  return n;
}

void DeviceTextFeed::Mark(uint64_t ticket) {
  for (auto it = out_.begin(); it != out_.end(); ++it) {
    if (it->ticket != ticket) continue;
    const Out o = *it;
    out_.erase(it);
    if (o.is_slot) {
      DfxCheck(dfx_textfeed_slot_consumed(h_, o.idx), "dfx_textfeed_slot_consumed");
      slot_held_[o.idx] = false;
      if (on_slot_free_) on_slot_free_(o.idx);
    } else {
      // (an unmarked entry was not begun again: BeginBatch would have thrown)
      int cur = -1;
      DfxCheck(dfx_textfeed_counts(h_, nullptr, nullptr, &cur), "dfx_textfeed_counts");
      DfxCheck(dfx_textfeed_consumed_back(h_, (cur - o.idx + nring()) % nring()),
               "dfx_textfeed_consumed_back");
      ring_out_[o.idx] = false;
    }
    return;
  }
  if (ticket >= next_ticket_)
    throw FeedProtocolError("text feed: a mark for a batch not handed out yet");
}

// src -> dst over up to nthreads threads; returns the number of '\n' bytes copied; blanks (a
// sized feed): also counts the bytes that bound the chunk's features: the ' ' and '\t' bytes
// (libsvm: a feature follows a blank) or, with colons, the ':' bytes (adfea: every feature
// holds one)
static size_t CopyCountLines(char* dst, const char* src, size_t bytes, int nthreads,
                             size_t* blanks = nullptr, bool colons = false) {
  std::vector<size_t> nblank(std::max(nthreads, 1), 0);
  size_t* const nb = blanks ? nblank.data() : nullptr;
  auto part = [nb, colons](char* d, const char* s, size_t n, int t = 0) {
    std::memcpy(d, s, n);
    size_t c = 0;
    if (nb) {
      size_t b = 0;
      if (colons) {
        for (const char *p = d, *e = d + n; p < e; ++p) {
          c += *p == '\n';
          b += *p == ':';
        }
      } else {
        for (const char *p = d, *e = d + n; p < e; ++p) {
          c += *p == '\n';
          b += (*p == ' ') | (*p == '\t');
        }
      }
      nb[t] = b;
      return c;
    }
    for (const char *p = d, *e = d + n; p < e; ++p, ++c) {
      p = static_cast<const char*>(std::memchr(p, '\n', e - p));
      if (!p) break;
    }
    return c;
  };
  struct Sum {  // the blanks of the parts, on every way out
    std::vector<size_t>& v;
    size_t* out;
    ~Sum() {
      if (!out) return;
      *out = 0;
      for (size_t x : v) *out += x;
    }
  } sum{nblank, blanks};
  const int T = (int)std::min<size_t>(std::max(nthreads, 1), 1 + bytes / (1 << 20));
  if (T <= 1) return part(dst, src, bytes);
  std::vector<size_t> cnt(T, 0);
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t) {
    const size_t a = bytes * t / T, b = bytes * (t + 1) / T;
    th.emplace_back([&, t, a, b]() { cnt[t] = part(dst + a, src + a, b - a, t); });
  }
  size_t total = 0;
  for (int t = 0; t < T; ++t) {
    th[t].join();
    total += cnt[t];
  }
  return total;
}

DeviceBatchReader::DeviceBatchReader(DeviceTextFeed* feed, const std::string& path,
                                     const std::string& format, int part, int nparts,
                                     size_t batch_size, size_t shuf_buf, float neg_sampling,
                                     int nthreads, size_t chunk_bytes)
    : feed_(feed),
      f_(feed->h()),
      reader_(path, format, part, nparts, chunk_bytes, nthreads, 0),
      train_(format != "criteo_test"),
      sized_(feed->sized()),
      valued_(feed->valued()),
      batch_size_(batch_size),
      nthreads_(nthreads < 1 ? 1 : nthreads) {
  DFX_HOST_CHECK(format == "criteo" || format == "criteo_test" || format == "libsvm" ||
                     format == "adfea",
                 "the device reader parses criteo, criteo_test, libsvm and adfea, not " + format);
  DFX_HOST_CHECK((format == "libsvm"  ? DFX_TEXT_LIBSVM
                  : format == "adfea" ? DFX_TEXT_ADFEA
                                      : DFX_TEXT_CRITEO) == feed->format(),
                 "the text feed was created for another format");
  DFX_HOST_CHECK(batch_size <= feed->batch_size() && shuf_buf <= feed->shuf_buf(),
                 "batch or shuffle buffer larger than the text feed's");
  if (batch_size_) {
    planner_.reset(new BatchPlanner(
        batch_size, shuf_buf, neg_sampling,
        [this](size_t* rows, const uint64_t** off, const float** lab) {
          return FetchChunk(rows, off, lab);
        },
        [this](const GatherOp& op) { Gather(op); }));
  }
  // a slot an earlier reader's batch still holds (handed out, not marked yet) stays away from
  // the loader; it comes here when it is marked.  This reader's own current chunk goes back at
  // the next FetchChunk, as ever.
  for (int s = 0; s < feed_->nslots(); ++s)
    if (!feed_->SlotHeld(s)) free_.push_back(s);
  feed_->OnSlotFree([this](int s) {
    if (s == cur_slot_) return;
    {
      std::lock_guard<std::mutex> lk(mu_);
      free_.push_back(s);
    }
    cv_.notify_all();
  });
  loader_ = std::thread([this]() { Load(); });
}

DeviceBatchReader::~DeviceBatchReader() {
  feed_->OnSlotFree(nullptr);
  {
    std::lock_guard<std::mutex> lk(mu_);
    stop_ = true;
  }
  cv_.notify_all();
  loader_.join();
  // parses still in flight read the slots' pinned text
  for (const Filled& c : submitted_) {
    int64_t stat[4];
    (void)dfx_textfeed_wait(f_, c.slot, stat, nullptr, nullptr, nullptr);
  }
}

void DeviceBatchReader::Load() {
  for (;;) {
    int slot;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [this]() { return stop_ || !free_.empty(); });
      if (stop_) return;
      slot = free_.front();
      free_.pop_front();
    }
    const char* data;
    size_t size;
    if (!reader_.NextRaw(&data, &size)) {
      {
        std::lock_guard<std::mutex> lk(mu_);
        eof_ = true;
      }
      cv_.notify_all();
      return;
    }
    char* dst = nullptr;
    DfxCheck(dfx_textfeed_text(f_, slot, (int64_t)size, &dst), "dfx_textfeed_text");
    const double t0 = Seconds();
    size_t blanks = 0;
    const size_t nl = CopyCountLines(dst, data, size, nthreads_, sized_ ? &blanks : nullptr,
                                     feed_->format() == DFX_TEXT_ADFEA);
    {
      std::lock_guard<std::mutex> lk(mu_);
      times_.copy += Seconds() - t0;
      filled_.push_back(Filled{slot, size, nl, blanks});
    }
    cv_.notify_all();
  }
}

void DeviceBatchReader::SubmitFilled(bool wait) {
  std::deque<Filled> take;
  {
    std::unique_lock<std::mutex> lk(mu_);
    if (wait) {
      const double t0 = Seconds();
      cv_.wait(lk, [this]() { return eof_ || !filled_.empty(); });
      times_.wait_text += Seconds() - t0;
    }
    take.swap(filled_);
  }
  for (const Filled& c : take) {
    // rows <= lines <= newlines: whole lines, the last one terminated (TextReader::NextRaw);
    // libsvm: a feature follows a blank; adfea: a feature holds a ':' (the loader counts either
    // for a sized feed only)
    DfxCheck(dfx_textfeed_submit(f_, c.slot, (int64_t)c.bytes, train_ ? 1 : 0,
                                 (int64_t)c.newlines, (int64_t)c.blanks),
             "dfx_textfeed_submit");
    submitted_.push_back(c);
  }
}

void DeviceBatchReader::ReleaseChunk() {
  if (cur_slot_ < 0) return;
  if (feed_->SlotHeld(cur_slot_)) {  // its batch is not marked yet: freed by the mark
    cur_slot_ = -1;
    return;
  }
  {
    std::lock_guard<std::mutex> lk(mu_);
    free_.push_back(cur_slot_);
  }
  cv_.notify_all();
  cur_slot_ = -1;
}

bool DeviceBatchReader::FetchChunk(size_t* rows, const uint64_t** off, const float** lab) {
  ReleaseChunk();
  SubmitFilled(false);
  if (submitted_.empty()) {
    SubmitFilled(true);
    if (submitted_.empty()) return false;  // the end of the part
  }
  const Filled c = submitted_.front();
  submitted_.pop_front();
  int64_t stat[4];
  const double t0 = Seconds();
  const int rc = dfx_textfeed_wait(f_, c.slot, stat, off, lab, &chunk_flag_);
  // adfea: the ':' bytes bound the features of every chunk inside the device's domain, so a
  // chunk that needs more (tokens without ':' at feature places) is outside it: handed back too.
  // Only nnz can be what overflowed: max_rows was the chunk's newline count and rows = newlines.
  const bool outside = rc == DFX_ERR_CAPACITY && feed_->format() == DFX_TEXT_ADFEA;
  if (!outside) DfxCheck(rc, "dfx_textfeed_wait");
  times_.wait_parse += Seconds() - t0;
  SubmitFilled(false);  // slots filled meanwhile: their parses run beside this chunk's batches
  *rows = (size_t)stat[0];
  if (stat[2] || outside) {  // needs_host: the host parser's rows into the same device arrays
    ++fallback_;
    char* text = nullptr;
    DfxCheck(dfx_textfeed_text(f_, c.slot, (int64_t)c.bytes, &text), "dfx_textfeed_text");
    reader_.ParseChunk(text, c.bytes, &host_blk_);
    static_assert(sizeof(size_t) == sizeof(uint64_t), "size_t offsets");
    DfxCheck(dfx_textfeed_upload(f_, c.slot, (int64_t)host_blk_.Size(),
                                 (int64_t)host_blk_.index.size(),
                                 reinterpret_cast<const uint64_t*>(host_blk_.offset.data()),
                                 host_blk_.index.data(),
                                 valued_ ? host_blk_.value.data() : nullptr,
                                 host_blk_.label.data(), &chunk_flag_),
             "dfx_textfeed_upload");
    *rows = host_blk_.Size();
    *off = reinterpret_cast<const uint64_t*>(host_blk_.offset.data());
    *lab = host_blk_.label.data();
  }
  cur_slot_ = c.slot;
  seq_slot_.push_back(c.slot);
  chunk_lab_ = *lab;
  chunk_off_ = *off;
  chunk_rows_ = *rows;
  return true;
}

// one copy of the plan; a sized feed: its nnz from the mirrored row lengths; a valued one: the
// flags carried along
void DeviceBatchReader::Gather(const GatherOp& op) {
  const bool from_shuf = op.src == GatherOp::kShuffle;
  const size_t nnz = sized_ ? MirrorRows(op, from_shuf) : 0;
  DfxCheck(dfx_textfeed_gather(f_, from_shuf ? -1 : seq_slot_[op.src], op.to_batch ? 1 : 0,
                               op.rows.empty() ? nullptr : op.rows.data(), (int64_t)op.begin,
                               (int64_t)op.n, (int64_t)op.r0, (int64_t)nnz),
           "dfx_textfeed_gather");
}

size_t DeviceBatchReader::MirrorRows(const GatherOp& op, bool from_shuf) {
  auto len = [&](size_t j) {
    return from_shuf ? (size_t)shuf_len_[j] : (size_t)(chunk_off_[j + 1] - chunk_off_[j]);
  };
  // a binary feed (adfea) mirrors no flags: none is ever set
  auto flag = [&](size_t j) {
    return valued_ ? (from_shuf ? shuf_flag_[j] : chunk_flag_[j]) : (uint8_t)0;
  };
  if (op.r0 == 0) {
    if (op.to_batch) {
      batch_valued_ = false;
    } else {
      shuf_len_.clear();
      shuf_flag_.clear();
    }
  }
  size_t nnz = 0;
  for (size_t i = 0; i < op.n; ++i) {
    const size_t j = op.rows.empty() ? op.begin + i : op.rows[i];
    nnz += len(j);
    if (op.to_batch) {
      batch_valued_ = batch_valued_ || flag(j);
    } else {
      shuf_len_.push_back((uint32_t)len(j));
      if (valued_) shuf_flag_.push_back(flag(j));
    }
  }
  return nnz;
}

bool DeviceBatchReader::Next() {
  if (!batch_size_) {  // every chunk one batch
    size_t rows = 0;
    const uint64_t* off;
    const float* lab;
    // held slots wait for their marks; with one slot left to circulate, marks are missing (or
    // the feed has fewer slots than the caller's deferral + 2): the loader would starve next
    if (feed_->SlotsHeld() >= feed_->nslots() - 1)
      throw FeedProtocolError(
          "text feed: every text slot but one holds a batch that was handed out and never "
          "marked (a missing Consumed / Mark, or fewer slots than the caller's deferral + 2)");
    do {
      if (!FetchChunk(&rows, &off, &lab)) return false;
    } while (rows == 0);
    bool valued = false;  // no flags (a Criteo feed), no loop
    for (size_t r = 0; chunk_flag_ && r < chunk_rows_ && !valued; ++r) valued = chunk_flag_[r];
    DfxCheck(dfx_textfeed_slot_batch(f_, cur_slot_, valued ? 1 : 0, &batch_),
             "dfx_textfeed_slot_batch");
    feed_->HandOutSlot(cur_slot_);
    slot_batch_ = true;
    return true;
  }
  const double t0 = Seconds();
  feed_->BeginBatch();
  times_.wait_step += Seconds() - t0;
  size_t rows, nnz;
  batch_valued_ = false;
  if (!planner_->Next(&rows, &nnz)) return false;
  DfxCheck(
      dfx_textfeed_batch_end(f_, (int64_t)rows, (int64_t)nnz, batch_valued_ ? 1 : 0, &batch_),
      "dfx_textfeed_batch_end");
  feed_->HandOutEntry();
  slot_batch_ = false;
  return true;
}

void DeviceBatchReader::Consumed() {
  feed_->MarkBack(0);
}

}  // namespace difacto
