// icikt_transfer.h -- how the library moves the caller's memory between host and device.  The one owner of that
// policy: nothing outside icikt_transfer.cpp reads the pinned buffers, the result pieces or the caller-pinned state.
// THE LIBRARY NEVER PAGE-LOCKS CALLER MEMORY (no hipHostRegister / hipHostUnregister anywhere in it, since round 4) and
// never hands pageable memory of 256 KB or more to an asynchronous copy: rounds 2 and 3 each saw one GPU memory-access
// fault at a host heap address inside a host entry, with per-call registrations of heap ranges that Python frees and
// reuses; DESIGN.md section 6 lists what a reading of that code found (registrations of neighbouring, non-page-aligned
// heap ranges set up and torn down independently while copies from a neighbour were in flight) and why the mode was
// deleted rather than repaired.
//   * the matrix: double-buffered column chunks through the library's pinned buffer (hipHostMalloc, kept from call to
//     call), host-side copies on a few threads, each chunk's pre-pass and pair-kernel launches enqueued before the
//     host stages the next chunk (MatrixUpload);
//   * pair lists: a bounce buffer in 8 MB pieces (upload_sync); results: one pinned buffer per array (download /
//     finish_stream);
//   * ICIKT_FLAG_HOST_PINNED: the caller states that the matrix and the result arrays of THIS call lie in memory it
//     has page-locked itself (hipHostMalloc / hipHostRegister): they are copied from and into directly.  The library
//     does not probe the caller's memory (hipPointerGetAttributes logs an error for every pageable pointer).
// Copies below kLockMin take the runtime's staging path, which does not touch the caller's pages from the GPU.
#ifndef ICIKT_TRANSFER_H
#define ICIKT_TRANSFER_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "icikt.h"

namespace icikt {
namespace host {

constexpr size_t kLockMin = (size_t)256 << 10;

// a pinned host buffer of the library's (hipHostMalloc), grown on demand (no copy in flight in it then) and kept
struct PinnedBuf {
  void* p = nullptr;
  size_t bytes = 0;
  hipError_t reserve(size_t need);
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf();
};

struct CopyPool;

// Everything a context uses to move caller memory (icikt_ctx::xfer)
struct Transfers {
  CopyPool* pool = nullptr;         // worker threads of the host-side copies (started on first use)
  PinnedBuf stage;                  // the matrix in column chunks (two halves), pair / task lists in 8 MB pieces
  hipEvent_t ev_copy[4] = {};       // [0]: the copy stream waits for the compute stream; [1..3]: behind chunk copies
  PinnedBuf tasks;                  // the task list the pipelined all-pairs path writes chunk by chunk
  // results of 256 KB or more: one pinned slot per array of a call (its position among the call's bounced downloads,
  // kept from call to call), copied in pieces with an event behind each, moved to the caller's array by finish_stream
  struct Piece { void* pinned; void* dst; size_t bytes; hipEvent_t ev; };   // ev may be null
  std::vector<PinnedBuf> out_slots;
  std::vector<Piece> pieces;
  size_t n_downloads = 0;           // bounced downloads of the current call
  std::vector<hipEvent_t> ev_out;   // events of the pieces in flight (a pool, reused from call to call)
  size_t ev_out_used = 0;
  bool host_pinned = false;         // the current call was made with ICIKT_FLAG_HOST_PINNED (PinnedScope)
  PinnedBuf csc_rec;                // a CSC upload's error record as the copy stream delivered it (ICIKT_CSC_ERR_WORDS words)
  bool csc_pending = false;         // ... and whether one is on its way / unread
  ~Transfers();
  hipError_t init();                // creates ev_copy
};

// For the duration of a host entry: the caller has page-locked the matrix and the result arrays when `flags` holds
// ICIKT_FLAG_HOST_PINNED, and they are copied from / into directly.  The only way that state is set.
struct PinnedScope {
  icikt_ctx* c;
  PinnedScope(icikt_ctx* ctx, uint32_t flags);
  ~PinnedScope();
  PinnedScope(const PinnedScope&) = delete;
  PinnedScope& operator=(const PinnedScope&) = delete;
};

// One upload of the caller's matrix in column chunks (upload_and_prepare's loop), on c->copy_stream.  The route:
//   staged (default)  through the library's pinned double buffer (a threaded host memcpy per chunk): the GPU never
//                     touches the caller's pages, and the library never page-locks them
//   in place          ICIKT_FLAG_HOST_PINNED on the call: the caller has page-locked the matrix itself; the copies are
//                     DMA straight out of it
//   small             matrices below kLockMin bytes take the runtime's own staging path
// A column-major float64 chunk lands in the device matrix itself.  Any other view (icikt_input) travels in ITS element
// type and order -- the same three routes, a strided copy of `rows` runs each -- into a device staging block of two
// halves (icikt_ctx::d_ingest), and k_ingest (icikt_ingest.hip) widens / transposes it into the device matrix on the
// copy stream, right behind its copy: stream order is what keeps a half from being overwritten before it has been read.
// A CSC view (icikt_csc_input) keeps the chunks -- ranges of columns, sized by the float64 matrix
// they become -- and the three routes; what travels for columns [c0, c0 + nc) is values[e0:e1] and indices[e0:e1],
// e0 = indptr[c0], e1 = indptr[c0 + nc], into a half of the same device staging block (values first, indices behind
// them at csc_val_cap), and k_scatter_csc (icikt_sparse.hip) writes the chunk's float64 columns behind the two copies.
// indptr is uploaded once, by begin(); the halves are sized by the chunk with the most entries (csc_max_nnz).
struct MatrixSrc {
  bool sparse = false, null = false;         // null: the caller passed no view at all (the entry checks say so)
  icikt_input v{};                           // dense: element type, order, leading dimension in elements
  icikt_csc_input s{};                       // sparse
  int64_t dst_col = 0;                       // the device column its column 0 lands at (icikt_cross_*: the second of two sources of one device matrix)
  MatrixSrc() = default;
  MatrixSrc(const icikt_input& d) : v(d) {}  // (a dense view converts: the callers that only know dense matrices)
  static MatrixSrc dense(const icikt_input* p) { MatrixSrc m; if (p) m.v = *p; else m.null = true; return m; }
  static MatrixSrc csc(const icikt_csc_input* p) { MatrixSrc m; m.sparse = true; if (p) m.s = *p; else m.null = true; return m; }
};
inline size_t index_bytes(int index_type) { return index_type == ICIKT_INDEX_I64 ? 8 : 4; }
// indptr[i] of a CSC view
inline int64_t csc_ptr(const icikt_csc_input& s, int64_t i) {
  return s.index_type == ICIKT_INDEX_I64 ? static_cast<const int64_t*>(s.indptr)[i] : (int64_t)static_cast<const int32_t*>(s.indptr)[i];
}

struct MatrixUpload {
  icikt_ctx* c;
  MatrixSrc x;                               // the caller's matrix
  int64_t n_feat, chunk_cols;                // rows of a column, columns of the largest chunk
  int64_t n_samp = 0, csc_max_nnz = 0;       // CSC: columns of the view (indptr holds n_samp + 1 offsets), entries of the fullest chunk
  size_t csc_val_cap = 0;                    // CSC: bytes of a staging half that hold values (the indices follow)
  bool staged = false, in_place = false;     // the route (in place: copies may still read the caller's matrix after the host went on)
  // picks the route for a span of `span` bytes, grows the staging buffers, and makes c->copy_stream (and `also`, when
  // not null) wait for the work already on c->stream: it may still read the device copy the chunks overwrite
  hipError_t begin(size_t span, hipStream_t also);
  // chunk k (0, 1, ... in order): columns [c0, c0 + nc) of the view into dst, column-major float64 with leading
  // dimension n_feat; *done is recorded behind the copy and, for a view that is not column-major float64, behind the
  // conversion (k_ingest) that follows it on the copy stream
  hipError_t copy(int k, double* dst, int64_t c0, int64_t nc, hipEvent_t* done);
  // CSC: the error record's way back, on the copy stream behind the last chunk (csc_verdict reads it once that stream
  // has been synchronised)
  hipError_t finish();
};
// After c->copy_stream has been synchronised: ICIKT_SUCCESS, or ICIKT_E_INVALID with the message of the entry the scatter
// kernel rejected during the upload the context made last (nothing to report when that upload was dense).
int csc_verdict(icikt_ctx* c);
// the message of an error record of k_scatter_csc (kind != 0)
std::string csc_message(const unsigned long long* rec);

inline size_t dtype_bytes(int dtype) { return dtype == ICIKT_DTYPE_F32 || dtype == ICIKT_DTYPE_I32 ? 4 : 8; }
inline bool view_is_plain(const icikt_input& v) { return v.dtype == ICIKT_DTYPE_F64 && v.order == ICIKT_ORDER_COL; }
inline icikt_input f64_view(const double* X, int64_t ld) { return icikt_input{X, ICIKT_DTYPE_F64, ICIKT_ORDER_COL, ld}; }
// bytes from the first to the last cell of columns [0, ncols) of an n_feat-row view
inline size_t view_span(const icikt_input& v, int64_t n_feat, int64_t ncols) {
  if (n_feat <= 0 || ncols <= 0) return 0;
  const size_t major = (size_t)(v.order == ICIKT_ORDER_ROW ? n_feat : ncols), minor = (size_t)(v.order == ICIKT_ORDER_ROW ? ncols : n_feat);
  return ((major - 1) * (size_t)v.ld + minor) * dtype_bytes(v.dtype);
}
// the view of columns [c0, ...) of v
inline icikt_input view_from_col(const icikt_input& v, int64_t c0) {
  icikt_input o = v;
  if (v.data) o.data = static_cast<const char*>(v.data) + (size_t)c0 * (v.order == ICIKT_ORDER_ROW ? (size_t)1 : (size_t)v.ld) * dtype_bytes(v.dtype);
  return o;
}

// H2D on c->stream, complete on return
int upload_sync(icikt_ctx* c, void* dst, const void* src, size_t bytes);
// D2H of a result array into the caller's buffer on c->stream (not synchronised: finish_stream delivers it)
int download(icikt_ctx* c, void* dst, const void* src, size_t bytes);
// Waits for c->stream AND delivers the bounced results piece by piece as their copies complete (a piece is moved to the
// caller's array while the next one still crosses PCIe); ok = false (something failed already) drops them.  Returns the
// stream's status.  On an error the caller's arrays may hold part of the results: the call fails.
hipError_t finish_stream(icikt_ctx* c, bool ok);
// The end of a host entry with status rc so far: finish_stream, then the other two streams (nothing may still touch the
// caller's memory when the entry returns).  Returns rc, or ICIKT_E_HIP "who: ..." when the stream failed.
int end_call(icikt_ctx* c, const char* who, int rc);
// the pinned buffer of the pipelined all-pairs path's task list, n int32 words at least
int task_staging(icikt_ctx* c, size_t n, int32_t** out);

}  // namespace host
}  // namespace icikt
#endif
