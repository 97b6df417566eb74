// icikt_transfer.cpp -- the library's copies of caller memory (the policy: icikt_transfer.h).
#include "icikt_transfer.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>

#include "icikt_host.h"

namespace icikt {
namespace host {

// Host-side copies into / out of the library's pinned buffers, on a few threads: one core moves ~10 GB/s, the c4
// matrix is 82 MB and PCIe takes it in 1.8 ms.  The threads belong to the context (started on first use, parked on a
// condition variable between copies: creating and joining seven threads per chunk cost ~0.2 ms a time, a millisecond of
// a c4 call); a copy is cut into parts that the workers and the calling thread take from a shared counter.
struct CopyPool {
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable cv_work, cv_done;
  const std::function<void(unsigned)>* job = nullptr;
  unsigned nparts = 0, done = 0;
  std::atomic<unsigned> next{0};
  unsigned long long gen = 0;
  bool stop = false;
  unsigned active = 0;   // workers that hold the current job (a copy is over when all parts are done AND nobody holds it)
  void worker() {
    unsigned long long seen = 0;
    for (;;) {
      const std::function<void(unsigned)>* f;
      unsigned n;
      {
        std::unique_lock<std::mutex> lk(m);
        cv_work.wait(lk, [&] { return stop || gen != seen; });
        if (stop) return;
        seen = gen; f = job; n = nparts;
        if (!f) continue;          // woke after the copy was over
        ++active;
      }
      unsigned mine = 0;
      for (unsigned i = next.fetch_add(1); i < n; i = next.fetch_add(1)) { (*f)(i); ++mine; }
      {
        std::lock_guard<std::mutex> lk(m);
        done += mine;
        --active;
        if (done == nparts && active == 0) cv_done.notify_one();
      }
    }
  }
  bool start(unsigned n) {
    try {
      while (th.size() < n) th.emplace_back(&CopyPool::worker, this);
    } catch (...) {}
    return !th.empty();
  }
  void run(unsigned n, const std::function<void(unsigned)>& f) {
    {
      std::lock_guard<std::mutex> lk(m);
      job = &f; nparts = n; done = 0; next.store(0); ++gen;
    }
    cv_work.notify_all();
    unsigned mine = 0;
    for (unsigned i = next.fetch_add(1); i < n; i = next.fetch_add(1)) { f(i); ++mine; }
    std::unique_lock<std::mutex> lk(m);
    done += mine;
    cv_done.wait(lk, [&] { return done == nparts && active == 0; });
    job = nullptr;
  }
  ~CopyPool() {
    { std::lock_guard<std::mutex> lk(m); stop = true; }
    cv_work.notify_all();
    for (auto& t : th) t.join();
  }
};

// `rows` pieces of `row_bytes`, strides in bytes (a contiguous copy: one row)
static void par_copy2d(Transfers& t, void* dst, size_t dst_stride, const void* src, size_t src_stride, size_t row_bytes, size_t rows) {
  const size_t total = row_bytes * rows;
  unsigned nt = (unsigned)std::min<size_t>(8, total / ((size_t)1 << 20));   // (12 threads measured slower than 8 on the pool's boxes)
  CopyPool* pool = nullptr;
  if (nt > 1) {
    if (!t.pool) { try { t.pool = new CopyPool(); } catch (...) { t.pool = nullptr; } }
    pool = t.pool;
    if (!pool || !pool->start(7)) pool = nullptr;
  }
  if (!pool) {   // small, or no threads to be had: one core does it all
    for (size_t r = 0; r < rows; ++r)
      memcpy(static_cast<char*>(dst) + r * dst_stride, static_cast<const char*>(src) + r * src_stride, row_bytes);
    return;
  }
  if (rows == 1) {   // a contiguous copy: pieces of ~1 MB
    const size_t piece = (size_t)1 << 20;
    const unsigned parts = (unsigned)((total + piece - 1) / piece);
    const std::function<void(unsigned)> f = [=](unsigned i) {
      const size_t off = (size_t)i * piece;
      memcpy(static_cast<char*>(dst) + off, static_cast<const char*>(src) + off, std::min(piece, total - off));
    };
    pool->run(parts, f);
    return;
  }
  const size_t per = std::max<size_t>(1, ((size_t)1 << 20) / std::max<size_t>(row_bytes, 1));   // rows per part: ~1 MB
  const unsigned parts = (unsigned)((rows + per - 1) / per);
  const std::function<void(unsigned)> f = [=](unsigned i) {
    const size_t r0 = (size_t)i * per, r1 = std::min(rows, r0 + per);
    for (size_t r = r0; r < r1; ++r)
      memcpy(static_cast<char*>(dst) + r * dst_stride, static_cast<const char*>(src) + r * src_stride, row_bytes);
  };
  pool->run(parts, f);
}
static void par_memcpy(Transfers& t, void* dst, const void* src, size_t bytes) { par_copy2d(t, dst, 0, src, 0, bytes, 1); }

hipError_t PinnedBuf::reserve(size_t need) {
  if (bytes >= need) return hipSuccess;
  if (p) (void)hipHostFree(p);
  p = nullptr;
  bytes = 0;
  // (write-combined memory was tried for the staging buffer, which the host only ever writes: no difference, round 4)
  const hipError_t e = hipHostMalloc(&p, need, hipHostMallocDefault);
  if (e == hipSuccess) bytes = need;
  return e;
}

PinnedBuf::~PinnedBuf() { if (p) (void)hipHostFree(p); }

Transfers::~Transfers() {
  for (hipEvent_t e : ev_copy) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ev_out) (void)hipEventDestroy(e);   // (only created ones are kept)
  delete pool;
}

hipError_t Transfers::init() {
  hipError_t e = hipSuccess;
  for (auto& ev : ev_copy)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  return e;
}

PinnedScope::PinnedScope(icikt_ctx* ctx, uint32_t flags) : c(ctx) { c->xfer.host_pinned = (flags & ICIKT_FLAG_HOST_PINNED) != 0; }
PinnedScope::~PinnedScope() { c->xfer.host_pinned = false; }

// a half of the staging buffers for a view that is not column-major float64: the largest chunk in the view's element
// type; for a CSC view the values and, behind them, the indices of the chunk with the most entries
static size_t ingest_half(const MatrixUpload& u) {
  if (u.x.sparse) return u.csc_val_cap + ((((size_t)u.csc_max_nnz * index_bytes(u.x.s.index_type)) + 255) & ~(size_t)255);
  return (((size_t)u.chunk_cols * (size_t)u.n_feat * dtype_bytes(u.x.v.dtype)) + 255) & ~(size_t)255;
}

hipError_t MatrixUpload::begin(size_t span, hipStream_t also) {
  Transfers& t = c->xfer;
  in_place = span >= kLockMin && t.host_pinned;
  staged = span >= kLockMin && !t.host_pinned;
  const bool plain = !x.sparse && view_is_plain(x.v);
  hipError_t e = hipSuccess;
  if (x.sparse) {
    // indptr, once (the library's own bounce buffer when it is large: it is not one of the arrays the caller may have
    // page-locked), and a clear error record; both on c->stream, which the copy stream is made to wait for below
    csc_val_cap = (((size_t)csc_max_nnz * dtype_bytes(x.s.dtype)) + 255) & ~(size_t)255;
    const size_t pbytes = (size_t)(n_samp + 1) * index_bytes(x.s.index_type);
    e = c->d_indptr.reserve(pbytes);
    if (e == hipSuccess) e = c->d_csc_err.reserve(icikt::ICIKT_CSC_ERR_WORDS);
    if (e == hipSuccess) e = t.csc_rec.reserve(icikt::ICIKT_CSC_ERR_WORDS * sizeof(unsigned long long));
    if (e != hipSuccess) return e;
    if (upload_sync(c, c->d_indptr.p, x.s.indptr, pbytes) != ICIKT_SUCCESS) return hipErrorUnknown;
    e = hipMemsetAsync(c->d_csc_err.p, 0, icikt::ICIKT_CSC_ERR_WORDS * sizeof(unsigned long long), c->stream);
    if (e != hipSuccess) return e;
  }
  const size_t half = plain ? (size_t)chunk_cols * (size_t)n_feat * sizeof(double) : ingest_half(*this);
  e = staged ? t.stage.reserve(2 * half) : hipSuccess;
  if (e == hipSuccess && !plain) e = c->d_ingest.reserve(2 * half);
  if (e == hipSuccess) e = hipEventRecord(t.ev_copy[0], c->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(c->copy_stream, t.ev_copy[0], 0);
  if (e == hipSuccess && also) e = hipStreamWaitEvent(also, t.ev_copy[0], 0);
  return e;
}

// chunk k of a CSC view: the two slices by the route of the upload, then the scatter
static hipError_t copy_csc(MatrixUpload& u, int k, double* dst, int64_t c0, int64_t nc) {
  icikt_ctx* c = u.c;
  Transfers& t = c->xfer;
  const icikt_csc_input& s = u.x.s;
  const int64_t e0 = csc_ptr(s, c0), e1 = csc_ptr(s, c0 + nc), cnt = e1 - e0;
  const size_t es = dtype_bytes(s.dtype), is = index_bytes(s.index_type), half = ingest_half(u);
  unsigned char* land = c->d_ingest.p + (size_t)(k & 1) * half;
  hipError_t e = hipSuccess;
  if (u.staged && k >= 2) e = hipEventSynchronize(t.ev_copy[1 + ((k - 2) % 3)]);  // the copy that last used this half
  if (e != hipSuccess) return e;
  if (cnt > 0) {
    const char* sv = static_cast<const char*>(s.values) + (size_t)e0 * es;
    const char* si = static_cast<const char*>(s.indices) + (size_t)e0 * is;
    if (u.staged) {
      char* stage = static_cast<char*>(t.stage.p) + (size_t)(k & 1) * half;
      par_memcpy(t, stage, sv, (size_t)cnt * es);
      par_memcpy(t, stage + u.csc_val_cap, si, (size_t)cnt * is);
      sv = stage;
      si = stage + u.csc_val_cap;
    }
    e = hipMemcpyAsync(land, sv, (size_t)cnt * es, hipMemcpyHostToDevice, c->copy_stream);
    if (e == hipSuccess) e = hipMemcpyAsync(land + u.csc_val_cap, si, (size_t)cnt * is, hipMemcpyHostToDevice, c->copy_stream);
  }
  if (e == hipSuccess)
    e = icikt::launch_scatter_csc(land, s.dtype, land + u.csc_val_cap, c->d_indptr.p, s.index_type, c0, e0, cnt, s.fill,
                                  u.n_feat, nc, dst, u.n_feat, c->d_csc_err.p, c->copy_stream);
  return e;
}

hipError_t MatrixUpload::copy(int k, double* dst, int64_t c0, int64_t nc, hipEvent_t* done) {
  Transfers& t = c->xfer;
  hipError_t e = hipSuccess;
  if (x.sparse) {
    e = copy_csc(*this, k, dst, c0, nc);
    *done = t.ev_copy[1 + (k % 3)];
    if (e == hipSuccess) e = hipEventRecord(*done, c->copy_stream);
    return e;
  }
  const icikt_input& v = x.v;
  const bool plain = view_is_plain(v), row = v.order == ICIKT_ORDER_ROW;
  const size_t es = dtype_bytes(v.dtype);
  // the chunk in the caller's memory: `runs` runs of run_bytes, ld_bytes apart (COL: a run is a column; ROW: a run is
  // the chunk's part of a row)
  const char* src = static_cast<const char*>(view_from_col(v, c0).data);
  const size_t ld_bytes = (size_t)v.ld * es;
  const size_t run_bytes = (size_t)(row ? nc : n_feat) * es, runs = (size_t)(row ? n_feat : nc);
  const size_t half = plain ? (size_t)chunk_cols * (size_t)n_feat * sizeof(double) : ingest_half(*this);
  // where it lands, runs packed: the device matrix itself, or a half of the device staging block
  void* land = plain ? static_cast<void*>(dst) : static_cast<void*>(c->d_ingest.p + (size_t)(k & 1) * half);
  if (staged) {
    char* stage = static_cast<char*>(t.stage.p) + (size_t)(k & 1) * half;
    if (k >= 2) e = hipEventSynchronize(t.ev_copy[1 + ((k - 2) % 3)]);  // the copy that last used this half
    if (e != hipSuccess) return e;
    par_copy2d(t, stage, run_bytes, src, ld_bytes, run_bytes, runs);
    e = hipMemcpyAsync(land, stage, runs * run_bytes, hipMemcpyHostToDevice, c->copy_stream);
  } else {
    e = hipMemcpy2DAsync(land, run_bytes, src, ld_bytes, run_bytes, runs, hipMemcpyHostToDevice, c->copy_stream);
  }
  if (e == hipSuccess && !plain)
    e = icikt::launch_ingest(land, v.dtype, v.order, row ? nc : n_feat, n_feat, nc, dst, n_feat, c->copy_stream);
  *done = t.ev_copy[1 + (k % 3)];
  if (e == hipSuccess) e = hipEventRecord(*done, c->copy_stream);
  return e;
}

hipError_t MatrixUpload::finish() {
  Transfers& t = c->xfer;
  if (!x.sparse) { t.csc_pending = false; return hipSuccess; }
  t.csc_pending = true;
  return hipMemcpyAsync(t.csc_rec.p, c->d_csc_err.p, icikt::ICIKT_CSC_ERR_WORDS * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost, c->copy_stream);
}

std::string csc_message(const unsigned long long* rec) {
  const std::string at = " (column " + std::to_string((long long)rec[1]) + ", entry " + std::to_string((long long)rec[2]) + ")";
  switch (rec[0]) {
    case icikt::ICIKT_CSC_BAD_ROW:
      return "X->indices: row index " + std::to_string((long long)rec[3]) + " outside [0, n_feat)" + at;
    case icikt::ICIKT_CSC_DUPLICATE:
      return "X->indices: duplicate entry (sum_duplicates) for row " + std::to_string((long long)rec[3]) + at;
    default:
      return "X->indptr: a column's offsets lie outside the arrays" + at;
  }
}

int csc_verdict(icikt_ctx* c) {
  Transfers& t = c->xfer;
  if (!t.csc_pending) return ICIKT_SUCCESS;
  t.csc_pending = false;
  const unsigned long long* rec = static_cast<const unsigned long long*>(t.csc_rec.p);
  if (!rec || rec[0] == 0) return ICIKT_SUCCESS;
  return fail(c, ICIKT_E_INVALID, "sparse matrix: " + csc_message(rec));
}

int upload_sync(icikt_ctx* c, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return ICIKT_SUCCESS;
  Transfers& t = c->xfer;
  if (bytes >= kLockMin) {
    // through the library's pinned bounce buffer, a chunk at a time (pair and task lists: the library's own vectors
    // or the caller's index arrays -- ICIKT_FLAG_HOST_PINNED speaks of the matrix and the result arrays only)
    const size_t cap = (size_t)8 << 20;
    HIPCHK(c, t.stage.reserve(std::min(bytes, cap)));
    for (size_t off = 0; off < bytes; off += cap) {
      const size_t m = std::min(cap, bytes - off);
      par_memcpy(t, t.stage.p, static_cast<const char*>(src) + off, m);
      hipError_t e = hipMemcpyAsync(static_cast<char*>(dst) + off, t.stage.p, m, hipMemcpyHostToDevice, c->stream);
      const hipError_t es = hipStreamSynchronize(c->stream);
      if (e == hipSuccess) e = es;
      if (e != hipSuccess) return fail(c, ICIKT_E_HIP, std::string("H2D copy (staged): ") + hipGetErrorString(e));
    }
    return ICIKT_SUCCESS;
  }
  hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
  const hipError_t es = hipStreamSynchronize(c->stream);       // the host range must outlive the copy
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(c, ICIKT_E_HIP, std::string("H2D copy: ") + hipGetErrorString(e));
  return ICIKT_SUCCESS;
}

int download(icikt_ctx* c, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return ICIKT_SUCCESS;
  Transfers& t = c->xfer;
  if (bytes >= kLockMin && !t.host_pinned) {
    // into a pinned buffer of the library's: the array's position among the call's bounced downloads picks it, so an
    // array keeps its buffer from call to call whatever the sizes of the arrays before it
    const size_t slot = t.n_downloads++;
    if (slot >= t.out_slots.size()) t.out_slots.resize(slot + 1);
    PinnedBuf& ps = t.out_slots[slot];
    HIPCHK(c, ps.reserve(bytes));
    // in pieces, an event behind each: finish_stream() moves a piece to the caller's array while the next ones are
    // still on their way (c4: 19 MB of results, 0.4 ms of PCIe and 0.25 ms of host copy that used to run one after the other)
    const size_t piece = std::max<size_t>((size_t)4 << 20, (bytes + 3) / 4);
    for (size_t off = 0; off < bytes; off += piece) {
      const size_t m = std::min(piece, bytes - off);
      HIPCHK(c, hipMemcpyAsync(static_cast<char*>(ps.p) + off, static_cast<const char*>(src) + off, m, hipMemcpyDeviceToHost, c->stream));
      hipEvent_t ev = nullptr;
      if (t.ev_out_used < t.ev_out.size()) ev = t.ev_out[t.ev_out_used];
      else if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) t.ev_out.push_back(ev);
      else { (void)hipGetLastError(); ev = nullptr; }
      if (ev) { t.ev_out_used += 1; HIPCHK(c, hipEventRecord(ev, c->stream)); }
      t.pieces.push_back(Transfers::Piece{static_cast<char*>(ps.p) + off, static_cast<char*>(dst) + off, m, ev});
    }
    return ICIKT_SUCCESS;
  }
  HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  return ICIKT_SUCCESS;
}

hipError_t finish_stream(icikt_ctx* c, bool ok) {
  Transfers& t = c->xfer;
  for (auto& b : t.pieces) {
    if (!ok) break;
    // (a piece without an event -- none could be created -- waits for everything enqueued so far)
    const hipError_t e = b.ev ? hipEventSynchronize(b.ev) : hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipGetLastError(); ok = false; break; }
    par_memcpy(t, b.dst, b.pinned, b.bytes);
  }
  t.pieces.clear();
  t.ev_out_used = 0;
  t.n_downloads = 0;
  return hipStreamSynchronize(c->stream);
}

int end_call(icikt_ctx* c, const char* who, int rc) {
  const hipError_t es = finish_stream(c, rc == ICIKT_SUCCESS);
  (void)hipStreamSynchronize(c->prep_stream);   // (a pipelined upload from page-locked memory is not waited for before)
  const hipError_t ec = hipStreamSynchronize(c->copy_stream);
  // a CSC upload whose error record is still unread (a pipelined upload from page-locked arrays): malformed input fails
  // the call now that its streams have drained
  if (c->xfer.csc_pending) {
    if (ec != hipSuccess || rc) c->xfer.csc_pending = false;   // (a call that has failed already keeps its own message)
    const int rv = csc_verdict(c);
    if (rv) return rv;
  }
  if (rc || es == hipSuccess) return rc;
  return fail(c, ICIKT_E_HIP, std::string(who) + ": " + hipGetErrorString(es));
}

int task_staging(icikt_ctx* c, size_t n, int32_t** out) {
  HIPCHK(c, c->xfer.tasks.reserve(n * sizeof(int32_t)));
  *out = static_cast<int32_t*>(c->xfer.tasks.p);
  return ICIKT_SUCCESS;
}

}  // namespace host
}  // namespace icikt
