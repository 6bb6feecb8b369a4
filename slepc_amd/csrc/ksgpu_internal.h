// Internal declarations of libksgpu (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include <string>
#include "../../include/ksgpu.h"
#include "ks_dict_pairs.h"

// ---- error plumbing ---------------------------------------------------------------------------
void ks_set_error(const char *fmt, ...);
// resident workgroups per CU of a kernel symbol; a query that fails is COUNTED (ks_runtime_info), reported once on stderr with the HIP runtimes the
// process maps, and answered with `fallback` - never silently (round 3's failures: profiles/r04_hip_runtime_probe.txt)
int ks_occupancy(const void *kernel, int block_threads, size_t lds_bytes, int fallback);
#define KS_FAIL(rc, ...) do { ks_set_error(__VA_ARGS__); return (rc); } while (0)
#define KS_CHECK(cond, rc, ...) do { if (!(cond)) KS_FAIL(rc, __VA_ARGS__); } while (0)
#define KS_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    ks_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); return KS_ERR_LIB; } } while (0)
#define KS_CALL(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

// ---- profiling ----------------------------------------------------------------------------------
struct KsProfSlot { long long launches = 0; double ms = 0.0; double bytes = 0.0; double hbm = 0.0; };
struct KsProfPending { hipEvent_t e0, e1; int kclass; int variant; double bytes; double hbm; int tag_col; int tag_slot; int tag_k; long long tag_n; bool done; double tag_extra = 0.0; };

// Host mailbox of the ops->gramschmidt slot (one per context, pinned coherent host memory): the update kernel's bookkeeping writes the scalars
// the slot returns here and stamps them with the call's sequence number; the host polls the stamp instead of waiting for the stream.
struct KsGsMail { double onrm, nrm; int fused, err; unsigned long long seq; };

// ---- communicator -------------------------------------------------------------------------------
#define KS_ONESHOT_MAX_RANKS 16
#define KS_ONESHOT_MAX_COUNT 128
#define KS_HALO_MAX_PEERS 16
struct KsComm {
  int rank = 0, size = 1;
  bool force_collectives = false;   // ks_ctx_set_debug(KS_DEBUG_FORCE_MULTI): take the multi-rank code path even with one rank (tests)
  // native RCCL (resolved with dlopen so that a process that already holds librccl reuses it)
  void *rccl_lib = nullptr;
  void *nccl_comm = nullptr;
  long long bcast_calls = 0; double bcast_seconds = 0.0;   // host wall time inside the broadcast of the projected problem (ks_comm_bcast_stats)
  char *ag_dev = nullptr; size_t ag_len = 0;   // device staging of the host allgather (kept: the projected solve is broadcast through it at every restart)
  // active provider (RCCL fills these with its own implementations)
  ks_comm_ops ops = {nullptr, nullptr, nullptr};
  void *user = nullptr;
  // one-shot allreduce over peer-mapped mailboxes (ks_comm_set_allreduce): every rank owns a mailbox in uncached device
  // memory, mapped by all the others (hipIpc between processes, the plain pointer inside one process)
  struct {
    bool enabled = false;
    unsigned seq = 0;                                    // stamp of the call, the same on every rank; travels inside every packet (never 0: what an untouched mailbox holds)
    unsigned par = 0;                                    // slot parity: flips on EVERY call (not derived from the stamp, which skips 0 when it wraps)
    unsigned long long *mine = nullptr;                  // [2 parities][KS_ONESHOT_MAX_RANKS][2 * KS_ONESHOT_MAX_COUNT] packets
    unsigned long long *peer[KS_ONESHOT_MAX_RANKS] = {}; // every rank's mailbox as mapped here (peer[rank] == mine)
    bool opened[KS_ONESHOT_MAX_RANKS] = {};              // mapped with hipIpcOpenMemHandle
    int *err_host = nullptr, *err_dev = nullptr;         // pinned: the sequence number of the first call that timed out, 0 = none
    int *err_local = nullptr;                            // the same word in device memory (what later kernels of this rank look at)
    long long timeout_ticks = 0;                         // wall_clock64 ticks (100 MHz) a rank waits for a packet before it gives up
  } oneshot;
  // peer-mapped halo exchange (ks_halo.hip): the error word a pack / unpack kernel raises when it gives up waiting (pinned, its device
  // address, and the copy in device memory later kernels of this rank look at)
  int *halo_err_host = nullptr, *halo_err_dev = nullptr, *halo_err_local = nullptr;
};

struct ks_ctx_s {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // multi-rank MatMult: the halo (pack + neighbour exchange) runs on its own stream under the diagonal-block product;
  // ev_x orders it after the producer of x on the main stream, ev_halo lets the off-diagonal rows wait for the ghosts
  hipStream_t halo_stream = nullptr; hipEvent_t ev_x = nullptr, ev_halo = nullptr;
  bool halo_overlap = true;
  // test hooks (ks_ctx_set_debug; each makes a test run the path the fast one replaces, or a multi-rank path on one rank)
  struct { bool no_fused_gs = false, no_mfma = false, no_spmv_dot = false, force_multi = false, no_dict_patterns = false, no_restart_fusion = false, no_dict_pairs = false, no_step_forward = false; unsigned oneshot_seq0 = 0; } dbg;
  long long nsync = 0;              // host synchronisations of the context's stream made by the library (ks_ctx_sync_count)
  long long basis_loads[2] = {0, 0};   // verdicts of ks_basis_loads_plain (ks_sweeps.cuh): plain loads [0], streaming loads [1]
  int num_cu = 256;
  char arch[64] = {0};
  size_t mem_total = 0;
  KsComm comm;
  // profiling
  bool prof_on = false;
  unsigned prof_mask = 0xffffffffu;   // classes that get HIP events when profiling is on
  KsProfSlot prof[KS_K_COUNT][KS_PROF_VARIANTS];
  std::vector<KsProfPending> pending;
  std::vector<hipEvent_t> event_pool;
  // split reductions (BVDotVecBegin/End ...): values queued by the Begin calls wait in `dev`; the first End performs ONE
  // allreduce over all of them (PetscSplitReduction's merged MPI_Allreduce) and the Ends hand the results out in order
  struct KsSplitEntry { int off, cnt, kind; };
  struct { double *dev = nullptr; int cap = 0, used = 0; std::vector<double> host; std::vector<KsSplitEntry> entries; size_t nread = 0; bool reduced = false; } split;
  // pinned host staging: [0, KS_PINNED_D2H_BYTES) results coming back (state, records, coefficient buffer), then two halves of
  // KS_PINNED_H2D_DOUBLES doubles for coefficient uploads (alternating; an event per half says when its last upload has left)
  double *h_pinned = nullptr; size_t h_pinned_len = 0;
  void *h_pinned_dev = nullptr;        // the same area as the device sees it (results written by a kernel instead of the copy engine); nullptr: not mapped
  hipEvent_t ev_h2d[2] = {nullptr, nullptr}; int h2d_next = 0;
  unsigned long long fetch_waited = 0;  // the newest stamp the host has seen: every launch enqueued before that results kernel has finished
  unsigned long long h2d_seq[2] = {0, 0}; bool h2d_busy[2] = {false, false};   // fetch_seq when a kernel was last enqueued to read that pinned half
  bool fetch_by_kernel = false;         // the batch enqueued by fetch_state_begin was written by the kernel (wait on its stamp) rather than by copies (wait on the event)
  unsigned long long fetch_seq = 0;     // stamp of the last batch of results a kernel wrote into the pinned area (its last word): the host polls it instead of waiting on the stream
  hipEvent_t ev_fetch = nullptr;        // marks the end of a batch of result copies that was enqueued ahead of further work (ks_gs.hip: fetch_state_begin / _end)
  KsGsMail *gs_mail = nullptr, *gs_mail_dev = nullptr;   // ops->gramschmidt slot: host mailbox and its device address (allocated on first use)
  unsigned long long gs_mail_seq = 0;
  hipEvent_t ev_mail = nullptr;         // behind the launch that writes the mailbox: what the host falls back on if the stamp does not show up
  long long nmailwait = 0;              // waits on the mailbox (instrumentation; they also count in nsync)
};

// every host wait on the context's stream goes through here, so that tests can assert that a call enqueues without waiting
// (a one-shot allreduce that gave up waiting shows here as a launch time-out, at the first wait after it)
static inline hipError_t ks_sync(ks_ctx ctx)
{
  ctx->nsync++;
  hipError_t e = hipStreamSynchronize(ctx->stream);
  const volatile int *os = ctx->comm.oneshot.err_host, *hh = ctx->comm.halo_err_host;
  return (e == hipSuccess && ((os && *os) || (hh && *hh))) ? hipErrorLaunchTimeOut : e;
}

int ks_prof_begin(ks_ctx ctx, int kclass, int variant, double alg_bytes, double hbm_bytes);   // records start event when profiling
int ks_prof_end(ks_ctx ctx, size_t index);
int ks_prof_flush(ks_ctx ctx);
struct KsProfScope {      // scopes may nest (an allreduce inside a bookkeeping slot): each remembers its own record
  ks_ctx ctx; bool on; size_t index = 0;
  KsProfScope(ks_ctx c, int kclass, double bytes, int variant = 0, double hbm = -1.0) : ctx(c), on(c->prof_on && ((c->prof_mask >> kclass) & 1u)) {
    if (on) { on = ks_prof_begin(c, kclass, variant, bytes, hbm < 0 ? bytes : hbm) == KS_SUCCESS; index = c->pending.empty() ? 0 : c->pending.size() - 1; }
  }
  ~KsProfScope() { if (on) ks_prof_end(ctx, index); }
  // tag the record of a speculative Gram-Schmidt slot so it can be re-filed once pass counts are known
  void tag(int col, int slot, int k, long long n, double extra = 0.0) { if (on && index < ctx->pending.size()) { auto &p = ctx->pending[index]; p.tag_col = col; p.tag_slot = slot; p.tag_k = k; p.tag_n = n; p.tag_extra = extra; } }
};
struct KsStepRec;
void ks_prof_resolve_gs(ks_ctx ctx, const KsStepRec *recs, int col0, int col1);   // re-file tagged records of columns [col0,col1]

int ks_allreduce_sum(ks_ctx ctx, double *dev_buf, int count);   // no-op when size==1
struct KsOneShotArgs { unsigned long long *peer[KS_ONESHOT_MAX_RANKS]; const unsigned long long *mine; int *err; int *err_local; long long timeout_ticks; unsigned seq, par; int me, size; };
bool ks_oneshot_next(ks_ctx ctx, int count, KsOneShotArgs *o);  // arguments of the next one-shot call, or false when the provider has to do it
int ks_oneshot_error(ks_ctx ctx);                               // KS_ERR_LIB once a one-shot allreduce has timed out (checked wherever the host has just waited)
void ks_oneshot_release(ks_ctx ctx);
int ks_comm_allgather_host(ks_ctx ctx, const void *send, int bytes, void *recv);
int ks_comm_exchange(ks_ctx ctx, int npeers, const int *peers, const void *dev_send, const int *send_off, const int *send_cnt,
                     void *dev_recv, const int *recv_off, const int *recv_cnt, int elem_bytes, hipStream_t stream = nullptr);   // nullptr: the context's stream
int ks_comm_bcast0_host(ks_ctx ctx, void *buf, int bytes);     // every rank leaves with rank 0's bytes (through the provider's host allgather)
int ks_ctx_halo_stream(ks_ctx ctx);                            // creates the halo stream and its events on first use
static inline bool ks_is_multi(ks_ctx ctx) { return ctx->comm.size > 1 || ctx->comm.force_collectives; }

// ---- Mat ----------------------------------------------------------------------------------------
struct ks_mat_s {
  ks_ctx ctx = nullptr;
  int n = 0;             // local rows
  int row_start = 0;     // first global row
  int n_global = 0;
  long long nnz = 0;     // local nonzeros (diag + offdiag blocks)
  // the CSR arrays the matrix was created from (global columns), kept on the host for KS_MAT_KEEP_CSR: what MatDuplicate / MatAXPY need (ks_mat_create_axpy)
  bool keep_csr = false; std::vector<int> k_rowptr, k_col; std::vector<double> k_val;
  ks_mat At = nullptr;                        // MatMultTranspose: the transpose, built on first use from the kept arrays (owned)
  ks_mat transpose_of = nullptr;              // set on such an At: the matrix that owns it. ks_mat_create_transpose hands the At out as a view; only its owner frees it
  // KS_MAT_SHARDED_TRANSPOSE (more than one rank): the matrix keeps its sorted ghost list and its pack list on the host, what the plan of the
  // transposed product is made from (ksc::sharded_transpose_plan) together with the kept CSR arrays. The At of such a matrix is the transposed
  // DIAGONAL block assembled on its own (no halo of its own) and carries the rest of the plan in `sht`; its product is mult_sharded_transpose (ks_spmv.hip)
  bool sharded_transpose = false; std::vector<int> h_ghosts, h_send_idx;
  struct ShT {
    int *o_rp = nullptr, *o_row = nullptr; double *o_val = nullptr; long long nnz_o = 0;   // transposed off-diagonal block: nghost rows of local row indices
    int *acc_rows = nullptr, *acc_ptr = nullptr, *acc_pos = nullptr; int nacc = 0;         // inverse of send_idx
    double *rsend = nullptr, *rrecv = nullptr;                                              // [nghost] sums for the ghosts' owners, [nsend] the peers' sums for this rank's rows
  } *sht = nullptr;
  // diagonal block (columns owned by this rank, LOCAL column indices)
  int *d_rowptr = nullptr; int *d_col = nullptr; double *d_val = nullptr; long long nnz_d = 0;
  int lanes_per_row = 8;
  // device layout of the diagonal block, chosen at assembly (choose_layout, ks_mat.hip): a KS_MAT_LAYOUT_* value (SHELL is shell_mult's)
  int layout = KS_MAT_LAYOUT_CSR;
  enum CsrForm : unsigned char { CSR_AUTO, CSR_VEC, CSR_REGS } csr_form = CSR_AUTO;   // the CSR kernel KSGPU_SPMV=csrvec / csrregs forces
  // sliced-ELL copy of the diagonal block (slice = 64 rows = one wavefront), chosen at assembly when the
  // padding it needs is small; val/col stored column-major inside a slice: entry j of row 64s+lane at (sp[s]+j)*64+lane
  int nslices = 0; int *s_ptr = nullptr; int *s_len = nullptr; int *s_col = nullptr; double *s_val = nullptr; long long s_entries = 0;
  // dictionary ELL (few distinct values and few distinct column offsets, rows of at most 32 entries): 2 bytes per entry
  int dict_w = 0; int dict_nval = 0, dict_noff = 0;
  unsigned short *dc_codes = nullptr; double *dc_val = nullptr; int *dc_off = nullptr;
  // row-pattern form of the same layout (at most 256 distinct rows): one byte per row, the index of its code word (dict_w 2-byte codes) in dc_pats;
  // dc_codes is then null. dc_rowpat is padded with zeros to a multiple of 256 rows.
  unsigned char *dc_rowpat = nullptr; unsigned short *dc_pats = nullptr; int dict_npat = 0;
  // pair form of the row-pattern form (ks_dict_pairs.h; decided once at assembly, build_dict_pairs): the bases, and per pattern the coefficient of every
  // candidate (base, d) and the bit mask of the candidates it has. The matrix bytes that stream are the same; which kernel runs is decided at launch
  // (16-byte aligned x and y, KS_DEBUG_NO_DICT_PAIRS) and counted in pr_launches / dc_row_launches (ks_mat_get_dict_pairs_info)
  bool pr_ok = false; ksp::PairArgs pr_args; double *pr_coef = nullptr; unsigned *pr_mask = nullptr; long long pr_launches = 0, dc_row_launches = 0;
  // offset-dictionary ELL: any values, few distinct column offsets: 1 byte per entry for the index, values in SELL order
  unsigned char *dc_codes8 = nullptr; double *dc_vals = nullptr;
  // XCD-sliced copy of the diagonal block for wide-scatter matrices (columns spread over a vector much larger than one
  // XCD's 4 MiB L2): the columns are cut into nslice = 8*P ranges; slice s is a CSR of its own (rows 0..n-1) and is
  // multiplied only by workgroups with blockIdx % 8 == s % 8, i.e. on one XCD, whose L2 then holds that range of x.
  // Every XCD writes a partial y; a second kernel adds the eight partials in fixed order.
  int nslice = 0, slice_cols = 0;
  int *sl_rowptr = nullptr; int *sl_col = nullptr; double *sl_val = nullptr; long long *sl_base = nullptr;   // [nslice][n+1], entries, device offsets [nslice+1]
  double *ypart = nullptr;                    // [8][n]
  double *mm_xi = nullptr;                    // block product, CSR interleaved form: [n][8] row-major copy of a pass's columns (ks_spmm.hip), allocated on first use
  // MatGetDiagonal / the infinity norm, taken before the binned, sliced and dictionary layouts release the CSR arrays (non-null: released)
  double *diag_cache = nullptr; double norm_inf_cache = -1.0;
  // Binned ("propagation blocking") copy of the diagonal block for wide-scatter matrices, the successor of the XCD-sliced one: the product
  // runs in two streaming phases with every random access in LDS. Columns are cut into bn_ns slices of bn_cs, rows into bn_wb wave-bins of
  // bn_wr. Entries are stored twice over: the 16-bit slice-local column in SLICE-major order (slice, wave-bin, row), the value and the 16-bit
  // bin-local row in BIN-major order (wave-bin, slice, row); a (slice, wave-bin) segment is contiguous in both, holds a multiple of 8
  // entries (padding entries with value 0 where needed) and so starts on a 64-byte boundary of the 8-byte streams. Phase 1 (a workgroup per slice, its piece of x in LDS) writes G = x[col] in bin-major
  // order; phase 2 (a wave per wave-bin, its rows of y in LDS) streams G, val and row and adds val * G into its rows.
  int bn_ns = 0, bn_cs = 0, bn_wb = 0, bn_wr = 0, bn_nwin = 0;
  long long bn_entries = 0;                   // entries incl. padding
  unsigned short *bn_col16 = nullptr, *bn_row16 = nullptr;
  double *bn_val = nullptr, *bn_g = nullptr;
  int *bn_off1 = nullptr;                     // [ns][wb + 1] start of segment (s, wb) inside slice s's stream
  int *bn_off2t = nullptr;                    // [ns][wb]     start of that segment in bin-major order
  int *bn_wseg = nullptr;                     // [ns][nwin]   segment in which the 1024-entry window of slice s begins
  long long *bn_sbase = nullptr;              // [ns + 1]     start of slice s in bn_col16
  int *bn_off2 = nullptr;                     // [wb][ns]     physical start of segment (wb, s): bin-major order GROUPED by phase-2 workgroup, [wb / 4][ns][wb % 4]
  int *bn_log2 = nullptr;                     // [wb][ns + 1] logical start of that segment inside its wave-bin (piece after piece); [ns] = entries of the wave-bin
  // Windowed CSR (KS_MAT_LAYOUT_WINDOW, the plan: ks_csr.h): d_rowptr and d_val stay as they are, d_col is replaced by a 16-bit code per entry of a
  // window block (slot * 64 + (col & 63) against the block's ascending list of 64-double segments of x, which the kernel stages in LDS) and by
  // the 32-bit columns of the direct blocks (more than WIN_SMAX segments) in wn_dcol, entry e at wn_dcol[wn_dbase[block] + e]
  unsigned short *wn_codes = nullptr;         // [nnz_d + CW_PAD]
  int *wn_dcol = nullptr;                     // [direct entries + gaps + CW_PAD]
  int *wn_segptr = nullptr, *wn_seg = nullptr, *wn_dbase = nullptr;      // [blocks + 1], [wn_segments], [blocks] (ksc::WIN_NOT_DIRECT: a window block)
  long long wn_blocks = 0, wn_direct_blocks = 0, wn_entries = 0, wn_direct_entries = 0, wn_segments = 0;
  // Block CSR (KS_MAT_LAYOUT_BSR, only from ks_mat_create_bsr; the plan: ks_csr.h): the diagonal block as bsr_nb block rows of bsr_bs x bsr_bs blocks - one
  // int per block row, one LOCAL block column per block, the values block after block in stored order, every block row-major. No per-entry index:
  // d_col and d_val are released
  int bsr_bs = 0, bsr_nb = 0; long long bsr_blocks = 0;
  int *bsr_rowptr = nullptr, *bsr_col = nullptr;    // [bsr_nb + 1], [bsr_blocks + CW_PAD]
  double *bsr_val = nullptr;                        // [bsr_blocks bs bs + CW_PAD]
  // off-diagonal block (columns owned by other ranks), compressed to ghost indices [0,nghost)
  int *o_rowptr = nullptr; int *o_col = nullptr; double *o_val = nullptr; long long nnz_o = 0;
  int nghost = 0;
  int *o_rows = nullptr; int n_orows = 0;     // rows that have off-diagonal entries (compressed row list)
  double *ghost = nullptr;                    // received halo values (nghost)
  // halo plan (size>1): peers, counts, send index lists
  std::vector<int> peers, send_cnt, recv_cnt, send_off, recv_off;
  int *send_idx = nullptr; int nsend = 0;     // local row indices to pack
  double *send_buf = nullptr;
  // peer-mapped halo (ks_mat_set_halo, ks_halo.hip): this rank's mailbox - [2 parities][nghost] doubles | flag[2][KS_HALO_MAX_PEERS] | ack[KS_HALO_MAX_PEERS],
  // uncached device memory - and the neighbours' mailboxes as mapped here; ridx[i] = this rank's index in peer i's own peer list
  struct { bool enabled = false; unsigned long long seq = 0; char *mine = nullptr; size_t bytes = 0; char *peer_base[KS_HALO_MAX_PEERS] = {}; bool opened[KS_HALO_MAX_PEERS] = {};
           int ridx[KS_HALO_MAX_PEERS] = {}, remote_off[KS_HALO_MAX_PEERS] = {}, remote_nghost[KS_HALO_MAX_PEERS] = {}; unsigned *tickets = nullptr; long long timeout_ticks = 0; } hp;
  // matrix-free operator (MATSHELL with MATOP_MULT): y = shell_mult(user, x); may synchronise the host
  int (*shell_mult)(void *user, const double *x_dev, double *y_dev) = nullptr;
  int (*shell_mult_t)(void *user, const double *x_dev, double *y_dev) = nullptr;      // MATOP_MULT_TRANSPOSE
  bool shell_nosync = false;                  // the callback only enqueues work on the context's stream: a Krylov run may be enqueued ahead through it
  void *shell_user = nullptr;
};
// Binned layout: constants and the dynamic LDS of its two kernels, shared by the build (ks_mat.hip: fit test) and the product (ks_spmv.hip: kernels, launch)
constexpr int BN_MAXSEG = 12;            // segments a 1024-entry window may touch on the fast path
constexpr int BN_CS_MAX = 9984;          // columns of a slice: 78 KB of LDS next to the two offset rows
constexpr int BN_SEG_PAD = 8;            // a (slice, wave-bin) segment holds a multiple of 8 entries (padding: value 0 into the spare accumulator): every segment then
                                         // starts on a 64-byte boundary of G / the values in both orders. Against padding to pairs only, same box: gather 385 -> 343-357 us,
                                         // reduce 511 -> 493 us with 2.5 % more entries (profiles/r03_ab_binned.txt); 4: 370-377 / 508, 16: 346-362 / 497
static inline size_t ks_binned_lds1(int cs, int wb) { return (size_t)cs * 8 + (size_t)(2 * wb + 1) * 4 + 16 + 16 * 2048; }   // gather: x piece, off1 row, off2t row (+ 2 KB of column codes per wave)
static inline size_t ks_binned_lds2(int wr) { return (size_t)4 * (wr + 1) * 8; }                                             // reduce: 4 x (wr + 1) accumulators
// Windowed CSR: rows of a block (one workgroup: a wave per 64 rows) and the segments of x its window holds (WIN_SMAX * 512 bytes of LDS next to the
// 17 KB the four waves stage their chunks in: three workgroups per CU). The choice: DESIGN section 16, profiles/r07_window_layout.txt.
#ifndef KS_WIN_ROWS
#define KS_WIN_ROWS 256
#endif
#ifndef KS_WIN_SMAX
#define KS_WIN_SMAX 64
#endif
constexpr int WIN_ROWS = KS_WIN_ROWS, WIN_SMAX = KS_WIN_SMAX;
static_assert(WIN_ROWS == 256 || WIN_ROWS == 64, "a block is one workgroup of four waves or one wave");
static_assert(WIN_SMAX >= 1 && WIN_SMAX * 64 <= 65536, "a code is slot * 64 + (col & 63) in 16 bits");
// Block CSR: a wave takes the block rows that fill at most 64 scalar rows, a workgroup four waves' worth per step; the values stream in chunks of whole
// blocks that fit 512 scalars (one more for the aligned start of an odd block size): four 16-byte loads per lane - and of at most 64 blocks, one block
// column per lane (bs = 2: 256 scalars). The choice: DESIGN section 31.
constexpr int BSR_BS_MIN = 2, BSR_BS_MAX = 8;
constexpr int bsr_wave_rows(int bs) { return 64 / bs; }
constexpr int bsr_group_rows(int bs) { return 4 * bsr_wave_rows(bs); }
constexpr int bsr_chunk_blocks(int bs) { return 512 / (bs * bs) < 64 ? 512 / (bs * bs) : 64; }
int ks_binned_prepare(size_t lds1, size_t lds2);            // lets the two kernels have that much dynamic LDS (they live in ks_spmv.hip)
// `variant` of a KS_K_SPMV profile record: which product kernel ran (bench.py and the profiles key on the values)
enum KsSpmvVariant { KS_SPMV_CSR = 0, KS_SPMV_SELL = 8, KS_SPMV_DICT = 16, KS_SPMV_ODICT = 17, KS_SPMV_BINNED = 18, KS_SPMV_WINDOW = 19,      // k_spmv_csr*, k_spmv_sell<4>, k_spmv_dict, k_spmv_odict, k_binned_*, k_spmv_window
                     KS_SPMM_DICT = 20, KS_SPMM_ODICT = 21, KS_SPMM_SELL = 22, KS_SPMM_CSR = 23, KS_SPMM_CSR_IL = 24,    // k_spmm_*; 24: k_spmm_pack + k_spmm_csr (interleaved)
                     KS_SPMV_BSR = 25, KS_SPMM_BSR = 26 };                                                                 // k_spmv_bsr, k_spmm_bsr
int ks_mat_get_diagonal_internal(ks_mat A, double *d_dev);
int ks_mat_mult_transpose_internal(ks_mat A, const double *x, double *y);
int ks_st_apply_transpose_internal(ks_st st, const double *x, double *y);
void ks_halo_release(ks_mat A);
int ks_halo_peer_exchange(ks_mat A, const double *x, hipStream_t hs);     // pack into the neighbours' mailboxes, unpack this rank's own (ks_halo.hip)
int ks_halo_add(hipStream_t st, int nacc, const int *acc_rows, const int *acc_ptr, const int *acc_pos, const double *rrecv, double *y);   // y[acc_rows[i]] += rrecv[acc_pos[..]] (ks_halo.hip)
int ks_mat_assemble_local(ks_ctx ctx, int n_local, int row_start, int n_global, const int *rowptr, const int *col, const double *val, ks_mat *out);   // a diagonal block on its own: no halo plan, no collective (ks_mat.hip)
bool ks_mat_has_transpose_across_ranks(ks_mat A);     // an assembled matrix created with KS_MAT_SHARDED_TRANSPOSE | KS_MAT_KEEP_CSR, or a view of one

int ks_mat_norm_inf_local(ks_mat A, double *val);           // max row sum of |a_ij| over this rank's rows

// ---- block Jacobi with ILU(0) blocks (ks_pc.hip): factors and level schedule from CSR arrays with global columns, y = U^-1 L^-1 x ----
struct KsIlu;
// transpose: also the plan of the transposed triangles of the same factors, y = L^-T U^-T x (the device bytes of the factors double)
int ks_pc_ilu_build(ks_ctx ctx, int n, int row_start, int bs, const int *rp, const int *col, const double *val, bool transpose, KsIlu **out);
int ks_pc_ilu_apply(ks_ctx ctx, const KsIlu *p, const double *in, double *out);      // enqueued; in != out
int ks_pc_ilu_apply_transpose(ks_ctx ctx, const KsIlu *p, const double *in, double *out);      // enqueued; in != out; needs the transposed plan
int ks_pc_ilu_apply_multi(ks_ctx ctx, const KsIlu *p, int ncols, const double *X, long long ldx, double *Y, long long ldy);   // enqueued; blocks do not overlap; every column the bits of ks_pc_ilu_apply
int ks_pc_ilu_multi_columns(ks_ctx ctx, const KsIlu *p);   // columns of a pass of the above (0: one at a time)
void ks_pc_ilu_free(KsIlu *p);

// ---- sparse LU with fill (ks_pc_lu.hip): Q P Q^T = L U from CSR arrays of the whole matrix (one rank), y = Q^T U^-1 L^-1 Q x -------------------
// A level of the triangular solves with at least this many rows is a launch of its own, a run of levels with fewer one launch of a single workgroup
// (where the value comes from). ks_st_pc_lu_get_info reports the value a set-up used.
constexpr int KS_LU_WIDE = 8;
struct KsLu;
struct KsLuInfo { int n, levelsL, levelsU, wide, wide_launches, narrow_launches, neg, pos; long long nnzL, nnzU, bytes; const int *perm; };
int ks_pc_lu_wide_threshold();
int ks_pc_lu_build(ks_ctx ctx, int n, const int *rp, const int *col, const double *val, int ordering, bool transpose, KsLu **out);   // KS_ERR_MAT_LU_ZRPVT, KS_ERR_MEM: nothing is left allocated
int ks_pc_lu_apply(ks_ctx ctx, const KsLu *p, const double *in, double *out);                 // enqueued; in != out
int ks_pc_lu_apply_transpose(ks_ctx ctx, const KsLu *p, const double *in, double *out);       // needs the transposed plan
int ks_pc_lu_apply_multi(ks_ctx ctx, const KsLu *p, int ncols, const double *X, long long ldx, double *Y, long long ldy);   // every column the bits of ks_pc_lu_apply
int ks_pc_lu_multi_columns();
void ks_pc_lu_info(const KsLu *p, KsLuInfo *out);     // perm: host array of the plan, valid while it lives
void ks_pc_lu_free(KsLu *p);

// ---- smoothed-aggregation multigrid (ks_pc_amg.hip): the hierarchy of ksc::amg_plan from CSR arrays of the whole matrix (one rank), y = one V-cycle on x ----
struct KsAmg;
struct KsAmgOptions { double theta = 0.0; int degree = 2, coarse_limit = 200, max_levels = 10; bool smooth = true; };
constexpr int KS_AMG_MAX_LEVELS = 16;
struct KsAmgInfo { int levels; int rows[KS_AMG_MAX_LEVELS]; long long nnz[KS_AMG_MAX_LEVELS]; double rho[KS_AMG_MAX_LEVELS]; double complexity; long long bytes; int launches; };
int ks_pc_amg_build(ks_ctx ctx, int n, const int *rp, const int *col, const double *val, const KsAmgOptions &opt, KsAmg **out);   // KS_ERR_ARG_WRONGSTATE, KS_ERR_MAT_LU_ZRPVT, KS_ERR_MEM, KS_ERR_ARG_OUTOFRANGE: nothing is left allocated
int ks_pc_amg_apply(ks_ctx ctx, const KsAmg *p, const double *in, double *out);                 // enqueued; in != out
int ks_pc_amg_apply_multi(ks_ctx ctx, const KsAmg *p, int ncols, const double *X, long long ldx, double *Y, long long ldy);   // passes of eight columns; every column the bits of ks_pc_amg_apply
int ks_pc_amg_multi_columns();
void ks_pc_amg_info(const KsAmg *p, KsAmgInfo *out);
// one level on the host (arrays of the plan, valid while it lives): its operator, and - every level but the last, else NULL - its prolongator and aggregate index
int ks_pc_amg_level(const KsAmg *p, int level, int *n, int *nagg, const int **arp, const int **acol, const double **aval, const int **prp, const int **pcol, const double **pval, const int **agg);
void ks_pc_amg_free(KsAmg *p);

// A solver of the ST whose scalars stay on the device (ks_ksp_resident.cuh). Its state block begins with this head: iterations done, the two flags of
// the end of the solve (done: ended without vector work, conv: ended after a sweep's vector work), why it ended, iterations that found it ended
struct KsKspHead { int its, done, conv, reason; long long gated; };
// What the ST keeps of such a solver: iterations enqueued per host read of the state; the device scratch and the pinned copy the host reads; launches of
// the solver's own kernels, host reads, iterations that found the solve ended (the get_stats triple)
struct KsResident { int check = 8; char *dev = nullptr; void *host = nullptr; long long sweeps = 0, waits = 0, gated = 0; };
constexpr size_t KS_RESIDENT_HEAD_BYTES = 256;   // the state and up to four sums of the ranks; three partials arrays follow
constexpr int KS_RESIDENT_PART_COLS = 3;
// BiCGStab(l) (ks_bcgsl.hip) sums a Gram matrix of up to 15 entries: a head of 512 bytes (its state and 18 sums of the ranks) and 18 partials columns
constexpr size_t KS_BCGSL_HEAD_BYTES = 512;
constexpr int KS_BCGSL_PART_COLS = 18;
constexpr int KS_BCGSL_MAX_ELL = 4;
// ---- ST: spectral transformation (ks_st.hip) ----------------------------------------------------
struct ks_st_s {
  ks_ctx ctx = nullptr;
  int type = KS_ST_SHIFT; bool type_set = false;   // type_set: chosen by the caller (STSetType), not a solver's default
  double sigma = 0.0; bool sigma_set = false;
  // STPRECOND with the infinite default shift GD asks for with the largest-* criteria (STSetDefaultShift(PETSC_MAX_REAL) davidson.c:80, precond.c:70-74),
  // ignored once the caller sets a shift. The set-up resolves it: the preconditioner is built on B alone (pc_on_b), or there is none (pc_identity)
  bool sigma_inf = false, pc_on_b = false, pc_identity = false;
  double nu = 0.0; bool nu_set = false;      // STCAYLEY antishift (defaults to sigma, cayley.c:140)
  ks_mat bil = nullptr;                       // STCAYLEY: shell matrix A + nu B, the bilinear form of symmetric problems (cayley.c:70-77)
  ks_mat A = nullptr, B = nullptr;            // borrowed
  double rtol = 1e-8; int max_it = 10000, restart = 30;   // KSP: SLEPC_DEFAULT_TOL (stsles.c:407), PETSc defaults
  int ksp_type = KS_KSP_GMRES;                // KSPGMRES (the default of the shell matrix mode), KSPBCGS, KSPPREONLY, KSPCG, KSPMINRES or KSPBCGSL
  bool ksp_type_set = false, rtol_set = false, max_it_set = false;   // chosen by the caller (ks_st_set_ksp_type, ks_st_set_ksp): a solver with KSP defaults of its own (JD) keeps off those
  int gmres_refine = KS_BV_ORTHOG_REFINE_NEVER;   // KSPGMRESSetCGSRefinementType: PETSc's default is classical Gram-Schmidt without refinement
  ks_bv Kb = nullptr;                         // BiCGStab work vectors (7 columns); CG's r, z, p, w are its first four, MINRES takes all seven
  // KS_KSP_CG and KS_KSP_MINRES, each with a check interval and statistics of its own (ks_st_cg_*, ks_st_minres_*); their work vectors are Kb's columns
  KsResident cg, mr;
  // KS_KSP_BCGSL: the same for BiCGStab(l), its check interval counted in cycles of l steps; its 2 l + 4 work vectors are a BV of its own
  // (r_0..r_l, u_0..u_l, rt and a scratch column for P x ahead of a block preconditioner), made at set-up when the type is set
  KsResident bl = KsResident{4};
  int bcgsl_ell = 2;
  ks_bv Kl = nullptr;
  bool jacobi_abs = false;                    // PCJacobiSetUseAbs: KS_PC_JACOBI scales by 1 / |diag(P)| (a positive definite M for MINRES on an indefinite P)
  ks_bv K = nullptr, W = nullptr;             // GMRES basis (restart+1 columns), work vectors (3 columns)
  double *dinv = nullptr;                     // Jacobi: 1/diag(P)
  int pc_type = KS_PC_JACOBI, pc_bs = 0;      // PCSetType on the KSP's PC: point Jacobi, or block Jacobi (dense inverses or ILU(0) factors) with blocks of pc_bs consecutive local rows
  double *binv = nullptr;                     // block Jacobi: row i holds the pc_bs coefficients of row i of its block's inverse (n x pc_bs, zero beyond a short last block)
  double *pcwork = nullptr;                   // block Jacobi: the vector the blocks are applied to (n)
  KsIlu *ilu = nullptr;                       // KS_PC_BJACOBI_ILU: the blocks' factors on the device (owned)
  KsLu *lu = nullptr;                         // KS_PC_LU: the factors of P on the device (owned)
  int lu_ordering = KS_ORDERING_ND;           // ks_st_pc_lu_set_ordering
  KsAmg *amg = nullptr;                       // KS_PC_AMG: the multigrid hierarchy of P on the device (owned)
  KsAmgOptions amg_opt;                       // ks_st_pc_amg_set_*
  int matmode = KS_ST_MATMODE_SHELL;          // STSetMatMode: how P = A - sigma B exists (shell: applied term by term; copy: assembled, stsolve.c:603-631)
  ks_mat Pmat = nullptr;                      // ST_MATMODE_COPY: the assembled P (owned)
  ks_mat op = nullptr;                        // shell matrix whose MatMult is STApply
  // ks_st_set_transpose_solves: set-up also prepares P^T (transposed views of A and B, or of the assembled P) and the transposed preconditioner.
  // The views belong to the matrices they view (ks_mat_create_transpose); nothing here is allocated with the switch off.
  bool tsolves = false;
  ks_mat At = nullptr, Bt = nullptr, PmatT = nullptr;
  int n = 0; bool ready = false;
  long long solves = 0, its = 0; double last_rnorm = 0.0;
};
bool ks_st_is_plain(ks_st st);                // shift with sigma = 0 on a standard problem: Op = A itself
int ks_st_setup_internal(ks_st st);
int ks_st_apply_internal(ks_st st, const double *x, double *y);
int ks_st_pc_apply_multi_internal(ks_st st, int ncols, const double *X, int ldx, double *Y, int ldy);   // set-up done, arguments checked by the caller
void ks_st_backtransform_internal(ks_st st, int n, double *eigr, double *eigi);
// The two KSPs of the ST (ks_st.hip) on any left-preconditioned operator: the ST's own M^-1 P, or the projected operator of the Jacobi-Davidson
// correction equation (ks_jd.hip). An operator says how M^-1 P x and the preconditioned residual are formed; the iterations are one copy.
struct KsKspOp {
  virtual ~KsKspOp() {}
  virtual int apply(const double *x, double *out) = 0;                              // out = M^-1 P x (enqueued)
  virtual int residual(const double *rhs, const double *y, double *out) = 0;        // out = M^-1 (rhs - P y); y NULL: out = M^-1 rhs
  // out = M^-1 P x, out being column jout of K, and *dot = (e, out) on the host: the application followed by BVDotVec unless the operator has the two in one
  virtual int apply_dot(const double *x, double *out, ks_bv K, int jout, const double *e, double *dot);
};
// K: GMRES basis (restart + 1 columns), Kb: BiCGStab's 7 vectors (the one the type needs); strict: not converging or breaking down is KS_ERR_NOT_CONVERGED
struct KsKsp { ks_ctx ctx; long long n; ks_bv K, Kb; double rtol; int max_it, restart; bool strict; long long *solves, *its; double *last_rnorm; };
int ks_ksp_gmres(const KsKsp &k, KsKspOp &op, const double *rhs, double *y);
int ks_ksp_bcgs(const KsKsp &k, KsKspOp &op, const double *rhs, double *y);
int ks_ksp_preonly(const KsKsp &k, KsKspOp &op, const double *rhs, double *y);     // KSPPREONLY: y = M^-1 rhs, one application, no residual, no test; K and Kb are not used
// CG (ks_cg.hip) and MINRES (ks_minres.hip) take P and M^-1 apart, which KsKspOp does not offer: their own entries on the ST, tr: the transposed side.
// Both keep their scalars on the device (ks_ksp_resident.cuh); the reasons a solve ends with are the solver's own, 1 being converged
int ks_ksp_cg(const KsKsp &k, ks_st st, bool tr, const double *rhs, double *y);
int ks_ksp_minres(const KsKsp &k, ks_st st, bool tr, const double *rhs, double *y);
int ks_ksp_bcgsl(const KsKsp &k, ks_st st, bool tr, const double *rhs, double *y);   // BiCGStab(l) (ks_bcgsl.hip), any P: st->bl, st->Kl, st->bcgsl_ell
// the device scratch of such a solver (its state, the ranks' sums, the sweeps' partials) and the pinned copy of the state the host reads
int ks_resident_alloc(KsResident *r, size_t head_bytes = KS_RESIDENT_HEAD_BYTES, int part_cols = KS_RESIDENT_PART_COLS);
void ks_resident_free(KsResident *r);
// w = P p but for one term: *v non-NULL on return means w += (*b) (*v) is still to be done (P applied term by term; the sweep behind the product adds it: k_cg_pw, k_minres_alfa, k_bcgsl_apply). tmp: W(:,1)
int ks_st_product_one_term_left(ks_st st, bool tr, const double *p, double *w, const double **v, double *b);
int ks_st_blocks_apply(ks_st st, const double *in, double *out, bool tr);      // out = M^-1 in for the preconditioners with kernels of their own
bool ks_st_pc_pointwise(ks_st st, const double **dinv);   // set-up done. true: no preconditioner (*dinv NULL) or point Jacobi (*dinv its diagonal); false: blocks (ks_st_pc_apply_multi_internal)
int ksk_lincomb(ks_ctx ctx, long long n, const double *s, double a, const double *u, double b, const double *v, double *out);   // out = s.*(a*u + b*v)   // diagonal of the local diagonal block (MatGetDiagonal)

// ---- BV -----------------------------------------------------------------------------------------
// Device-resident Gram-Schmidt state (one per BV).  Written by the 1-block bookkeeping kernel,
// read by the sweep kernels; lets a whole Krylov run be enqueued with no host round trip.
struct KsGsState {
  int active;         // 0 after breakdown/error: every later kernel of the run is a no-op
  int do_update;      // coefficients c are ready: the next update kernel must apply them
  int fuse_dot;       // that update must also produce the partial dots of the next pass (or v'.v')
  int scale_now;      // that update is the final one: multiply by alpha while writing
  int expl;           // estimated norm^2 <= 0: explicit norm needed after the update (bvorthog.c:126)
  int pending_scale;  // final scaling still to be applied by the stand-alone scale kernel
  int pass;           // passes done for the current column
  int err;            // sticky error (KS_ERR_USER_INPUT: invalid inner product)
  int lindep;         // result for the current column
  int more_;          // another pass follows the pending update (bvorthog.c:179 loop condition)
  int halt_col;       // >=0: column whose orthogonalization needs slots beyond the optimistic program (host completes it)
  int store_now;      // the pending update writes the vector back (final update, or an explicit norm follows); a fused pass that
                      // only feeds the next pass's dots keeps its result in registers (writes cost ~5 read-columns of HBM time)
  int store_prev;     // the previous update of this column stored: the coefficients applied so far are in memory
  int npend;          // passes whose coefficients are not in memory yet: the next update applies pend[0..npend) one after the other
  int pgrid;          // gridDim.x of the sweep that last wrote `partials` (their stride and count): written by that sweep, read by the
                      // reduction, so a completion program enqueued after later columns' (gated-off) sweeps still reduces with the right grid
  double onrm, nrm, alpha;
  long long passes_total;
};
struct KsStepRec { double nrm, onrm; int passes, lindep, expl, col; };
// Forward form of the final update (ks_gs.hip): the device words of a BV's forward launches and the gate the ordinary product and
// dot sweep behind such a launch carry. Words: [KS_FWD_TAKEN] epoch of the launch whose bookkeeping chose the forward A-phases, [KS_FWD_ABORT] epoch of
// a launch in which a wait ran out of budget, then three running counts: launches that took the form, launches that gave up, fallback products that ran.
enum { KS_FWD_TAKEN = 0, KS_FWD_ABORT = 1, KS_FWD_NTAKEN = 2, KS_FWD_NABORT = 3, KS_FWD_NFALLBACK = 4, KS_FWD_WORDS = 8 };
struct KsFwdGate { unsigned *ctl = nullptr; unsigned epoch = 0; };      // ctl == nullptr: no gate. The gated launch does nothing iff ctl[TAKEN] == epoch && ctl[ABORT] != epoch

struct ks_bv_s {
  ks_ctx ctx = nullptr;
  int n = 0, N = 0, m = 0, l = 0, k = 0, nc = 0, ld = 0;
  int orthog_type = KS_BV_ORTHOG_CGS, orthog_ref = KS_BV_ORTHOG_REFINE_IFNEEDED, orthog_block = KS_BV_ORTHOG_BLOCK_GS;
  ks_mat matrix = nullptr;   // inner-product matrix B of BVSetMatrix (positive definite), borrowed; nullptr = standard
  int matmult = KS_BV_MATMULT_VECS;   // BVSetMatMultMethod: how the products of a block of this BV's columns run (ksb_matmult_block)
  double *Bx = nullptr;      // B*x of the vector an inner product is being taken with (BV_IPMatMult bvimpl.h:147-158)
  bool fetch_pending = false; size_t fetch_coefs = 0;     // result copies of the last enqueued column are on their way (gs_enqueue_column with early copies)
  // ops->gramschmidt slot, pass chaining (ks_bv_set_state): the last pass on column `col` left the next pass's dots in `partials`; they are used
  // only if the caller's state token is still `token_at` and no sweep of this BV has rewritten the partials since
  struct { bool armed = false, valid = false; unsigned long long token = 0, token_at = 0; int col = -1, pass_idx = 0; long long chained = 0, fresh = 0; } spec;
  double *pend = nullptr;    // [3][KS_PSTRIDE] coefficients of the passes since the vector was last written back (what the next update applies, pass by pass)
  double orthog_eta = 0.7071;
  bool fused_gs = true;      // the device-resident Gram-Schmidt program may be used (the no_fused_gs test hook is read when the BV is created)
  double deftol = 10 * 2.220446049250313e-16;
  double *array = nullptr;      // m*ld
  double *buffer = nullptr;     // (nc+m)*m ; column 0 = scratch c
  bool own_buffer = true;       // false: adopted from the caller (ks_bv_set_buffer: the device array of the reference's bv->buffer Vec)
  double *buffer_own = nullptr; // the library's own allocation while an adopted one is in use
  double *partials = nullptr;   // [KS_MAX_BLOCKS][KS_PSTRIDE] block partial sums: the CURRENT one of two buffers (an update kernel that carries the
                                // bookkeeping reads the current one in its prologue while its fused dots go to the other; the host swaps the pointers)
  double *partials_alt = nullptr, *partials_base = nullptr;
  double *coef = nullptr;       // device scratch for host-provided q / Q (max(m*m, ...))
  double *hc = nullptr;         // device h,c arrays for orthogonalizevec (2*(nc+m))
  double *cw = nullptr;         // [nc+m+1] wide bases (more than 64 previous columns): the pass's reduced dots, chunk after chunk
  double *cred = nullptr;       // [KS_PSTRIDE] multi-rank: the pass's dots summed over blocks and ranks, read by every workgroup of the update kernel
                                // (not the buffer's scratch column: workgroup 0 writes H(:,0) there while the others may still be reading)
  size_t coef_len = 0;
  KsGsState *gs = nullptr, *gs_alt = nullptr, *gs_base = nullptr;   // current / other device state (same ping-pong), allocation
  KsStepRec *recs = nullptr;    // m records (one per column)
  long long passes_total_host = 0; int passes_last_host = 0;
  int row_start = 0;            // first global row (reproducible random)
  int sweep_dir = 0;            // direction of the next row sweep over the basis: consecutive sweeps alternate (forward / backward), so each starts
                                // on the rows the previous one left in the Infinity Cache
  int last_grid = 1;            // grid size of the sweep LAUNCHED last (profiling byte counts, and reductions that directly follow their sweep); the
                                // Gram-Schmidt bookkeeping reads the grid from KsGsState::pgrid instead
  double *panel = nullptr; size_t panel_len = 0;   // block partials of the MFMA panel dot (grid x 64 x 64 max)
  // Deferred final update (ks_bv_set_defer_final): the last column of an enqueued Krylov run keeps its final CGS update back. Its bookkeeping has run
  // (k_gs_finish: state, pend, buffer column and record are complete), the update itself is still to be applied to column `col` against the
  // k = nc + col columns before it, in sweep direction `rev` (taken, and toggled, where the update would have been launched). Whoever touches
  // column data or Gram-Schmidt state next flushes it (ksb_flush); the restart (ksb_restart) applies it inside the restart product instead.
  struct { bool want = false, pending = false, one_pass = false; int col = 0, k = 0, rev = 0; long long flushes = 0, fused = 0; } defer;
  // Forward form of the final update: per-tile flags (never reset: a launch's epoch is its flag value, epochs only grow and are never 0), the control
  // words, the gate of the launches enqueued behind the newest forward launch (gate: what ksk_dot reads while enqueue_dots runs under it), the test
  // hooks (ks_bv_step_forward_hooks) and the reason of the last refusal
  struct { unsigned *flags = nullptr; size_t nflags = 0; unsigned *ctl = nullptr; unsigned epoch = 0; KsFwdGate next, gate; long long enqueued = 0;
           int force = 0, force_grid = 0, abort_wg = -1, lag_odd = 0; long long budget = -1; const char *why = ""; } fwd;
};

constexpr size_t KS_PINNED_D2H_BYTES = 65536;
constexpr size_t KS_PINNED_STAMP_OFF = KS_PINNED_D2H_BYTES - 64;      // the results' stamp (8 bytes); results may use the area below it
constexpr size_t KS_PINNED_H2D_DOUBLES = 4096;
constexpr int KS_MAX_COLS   = 64;     // max columns handled by the register-tiled sweeps (k+1 <= 64)
constexpr int KS_PSTRIDE    = 72;     // doubles per block in the partials array
constexpr int KS_MAX_BLOCKS = 4096;

static inline double *ks_bv_col(ks_bv bv, int j) { return bv->array + (size_t)(bv->nc + j) * bv->ld; }

// kernel launchers (ks_bv_kernels.hip / ks_gs.hip)
int ksk_dot(ks_bv bv, const double *A, int lda, int ncols, const double *y, bool gate);      // partials <- A(:,0:ncols)^T y
int ksk_reduce_partials(ks_bv bv, int ncols, double *out_dev);                                // out[i] = sum_b partials[b][i]
int ksk_multvec(ks_bv bv, const double *A, int lda, int ncols, double alpha, double beta, const double *q_dev, double *y, const KsGsState *gate = nullptr);
int ksk_scale(ks_ctx ctx, double *x, size_t n, double alpha);
int ksk_copy(ks_ctx ctx, const double *src, double *dst, size_t n);

int ks_mat_mult_internal(ks_mat A, const double *x, double *y, const double *rowscale = nullptr, const KsFwdGate *gate = nullptr);   // rowscale: y = rowscale .* (A x) where the layout can fold it into its last pass (else the caller scales)
bool ks_mat_can_rowscale(ks_mat A);
int ks_mat_mult_multi_internal(ks_mat A, int ncols, const double *X, int ldx, double *Y, int ldy);   // Y(:,j) = A X(:,j), j < ncols (ks_spmm.hip)
int ksb_matmult_block(ks_bv method_bv, ks_mat A, const double *X, int ldx, double *Y, int ldy, int ncols);   // BVMatMult's block product under method_bv's method
int ks_mat_mult_dot_fused(ks_mat A, ks_bv bv, const double *x, int jy, bool gate, bool *done);   // y = A x inside the dot sweep of column jy (ks_spmv.hip); *done = false: not applicable                                 // the product can take a row scaling in the same launches
int ks_bv_orthonormalize_coefs(ks_bv bv, int j, double *H, double *norm, int *lindep);
bool ks_bv_orthonormalize_can_split(ks_bv bv);
int ks_bv_orthonormalize_enqueue(ks_bv bv, int j);
int ks_bv_orthonormalize_collect(ks_bv bv, int j, double *H, double *norm, int *lindep, int *late_completion);
int ksb_ipmatmult(ks_bv bv, const double *x, const double **z);   // z = x, or B*x (in bv->Bx) when a matrix is set
int ksb_norm_b(ks_bv bv, const double *x, double *val);            // sqrt(x' B x) with the BV_SafeSqrt check (BVNorm_Private)
int ksb_dot_range(ks_bv X, int xs, int xe, ks_bv Y, int ys, int ye, double *M, int ldm);          // M(ys:ye,xs:xe) = Y(:,ys:ye)^T X(:,xs:xe)
int ksb_mult_range(ks_bv Y, int ys, int ye, double alpha, double beta, ks_bv X, int xs, int xe, const double *Q, int ldq);
int ksb_flush_pending(ks_bv bv);                                   // applies a deferred final update now (ks_gs.hip)
static inline int ksb_flush(ks_bv bv) { return (bv && bv->defer.pending) ? ksb_flush_pending(bv) : KS_SUCCESS; }   // first line of every entry that touches column data or Gram-Schmidt state
int ksb_restart(ks_bv V, const double *Q, int ldq, int s, int e, int src, int dst);   // BVMultInPlace(V,Q,s,e) then BVCopyColumn(V,src,dst); one launch with a pending update on src (ks_bv.hip)
int ksb_stage_coefs(ks_bv bv, const double *host, size_t len, double **dev);
// the fused restart kernel (ks_panel.hip): pending update of column src (k previous columns from V0, coefficients / state as k_gs_finish left them), product
// of the kin active columns A with Q into C(:,0:nout), the updated vector to columns src and dst
int ksp_restart_fused(ks_bv bv, const double *V0, int k, double *vsrc, double *vdst, const double *A, int kin, const double *Qdev, int ldq, int nout, double *C);
// MFMA f64 panel contractions (ks_panel.hip)
int ksp_dot_mfma(ks_bv bv, const double *Y, int ldy, int my, const double *X, int ldx, int nx, int n, double *M_dev);
int ksp_mult_mfma(ks_ctx ctx, int kclass, const double *A, int lda, int n, int kin, const double *Qdev, int qsk, int qsi, int nout,
                  double alpha, double beta, double *C, int ldc);
int ks_sweep_grid(ks_ctx ctx, int n, int vec);
int ks_sweep_grid_for(ks_ctx ctx, int n, int vec, const void *kernel, int force_per_cu);   // resident-blocks grid of one kernel symbol   // blocks of a row sweep (shared by every sweep kernel so partials line up)
