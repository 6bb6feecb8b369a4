/*
 * ksgpu.h -- C ABI of libksgpu: MI355X (gfx950) kernels for the SLEPc EPS Krylov-Schur hot path.
 *
 * Drop-in boundary.  Each entry point replaces one slot of the reference's plugin interfaces on raw
 * pointers (no PETSc types, no torch types).  Citations are SLEPc 3.22.2 paths (file:line):
 *
 *   struct _BVOps (include/slepc/private/bvimpl.h:25-61)        ->  ks_bv_*  below
 *   MatMult(Mat,Vec,Vec) reached through the ST shell
 *       (src/sys/classes/st/interface/stsolve.c:16-25,244-259)    ->  ks_mat_mult
 *   BVMatArnoldi / BVMatLanczos (bv/interface/bvkrylov.c:56,165)  ->  ks_bv_matarnoldi / ks_bv_matlanczos
 *   EPSSetOperators/EPSSolve/EPSGetEigenpair/EPSComputeError
 *       (src/eps/interface/epssetup.c:450, epssolve.c:119,406,742) ->  ks_eps_*
 *
 * Conventions (mirror the reference):
 *   - every function returns an int error code, 0 = success; non-zero values reuse PETSc's
 *     PetscErrorCode numbers (KS_ERR_*), so an adapter can `return (PetscErrorCode)rc;`
 *   - scalars are real double (PetscScalar), indices 32-bit int (PetscInt default build)
 *   - BV storage is ONE device array of (nc+m)*ld doubles, column-major, like BVSVEC
 *     (src/sys/classes/bv/impls/svec/svec.c:397-565); every op acts on the active window
 *     [l,k) at array+(nc+l)*ld (svec.c:30,47,124); nc constraint columns sit in front (ks_bv_insert_constraints)
 *   - Q / M / H arguments are caller-owned HOST column-major arrays, replicated on all ranks
 *     (bvops.c:33-36); q / m coefficient arrays are host arrays, NULL means "use the BV's
 *     device-resident buffer Vec" exactly as in BVMultVec/BVDotVec (svec.c:46,123)
 *   - numerical conditions (lindep, breakdown) are flags, not errors (bvkrylov.c:92-97)
 *   - single-threaded per context, collective across ranks: every rank calls in the same order
 *   - all device work is enqueued on the context's HIP stream; functions that return a host
 *     value synchronise that stream, the others do not.
 */
#ifndef KSGPU_H
#define KSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (PETSc numbering) ---------------------------------------------------------- */
#define KS_SUCCESS              0
#define KS_ERR_MEM             55
#define KS_ERR_SUP             56
#define KS_ERR_ORDER           58
#define KS_ERR_ARG_SIZ         60
#define KS_ERR_ARG_IDN         61
#define KS_ERR_FILE_OPEN       65
#define KS_ERR_FILE_UNEXPECTED 79
#define KS_ERR_ARG_WRONG       62
#define KS_ERR_ARG_OUTOFRANGE  63
#define KS_ERR_MAT_LU_ZRPVT    71   /* zero pivot in a block of the block-Jacobi preconditioner */
#define KS_ERR_USER_INPUT      95   /* BV_SafeSqrt "Invalid inner product" bvimpl.h:137 (PETSC_ERR_USER_INPUT; 71, used until round 3, is PETSC_ERR_MAT_LU_ZRPVT) */
#define KS_ERR_ARG_WRONGSTATE  73
#define KS_ERR_ARG_INCOMP      75
#define KS_ERR_LIB             76   /* HIP / RCCL runtime failure (PetscCallHIP analogue) */
#define KS_ERR_PLIB            77
#define KS_ERR_CONV_FAILED     82
#define KS_ERR_ARG_NULL        85
#define KS_ERR_NOT_CONVERGED   91   /* inner linear solve (KSPSetErrorIfNotConverged, stsles.c:58) */
#define KS_ERR_GPU             97   /* no usable gfx950 device */

const char *ks_error_string(int rc);
const char *ks_last_error_message(void);     /* detail of the last failure on this thread */

typedef struct ks_st_s  *ks_st;    /* spectral transformation: the operator of the Krylov expansion */
typedef struct ks_ctx_s *ks_ctx;   /* device + stream + communicator + profiling state            */
typedef struct ks_mat_s *ks_mat;   /* sparse operator (CSR / AIJ), row block owned by this rank   */
typedef struct ks_bv_s  *ks_bv;    /* basis vectors                                               */
typedef struct ks_eps_s *ks_eps;   /* Krylov-Schur eigensolver driver                             */

/* enums mirror include/slepcbv.h, include/slepceps.h, PETSc NormType */
enum { KS_BV_ORTHOG_CGS = 0, KS_BV_ORTHOG_MGS = 1 };
enum { KS_BV_ORTHOG_REFINE_IFNEEDED = 0, KS_BV_ORTHOG_REFINE_NEVER = 1, KS_BV_ORTHOG_REFINE_ALWAYS = 2 };
/* BVOrthogBlockType, include/slepcbv.h */
enum { KS_BV_ORTHOG_BLOCK_GS = 0, KS_BV_ORTHOG_BLOCK_CHOL = 1, KS_BV_ORTHOG_BLOCK_TSQR = 2, KS_BV_ORTHOG_BLOCK_TSQRCHOL = 3, KS_BV_ORTHOG_BLOCK_SVQB = 4 };
enum { KS_NORM_1 = 0, KS_NORM_2 = 1, KS_NORM_FROBENIUS = 2, KS_NORM_INFINITY = 3 };
/* EPSWhich, include/slepceps.h:109-119 (same numbering; TARGET_IMAGINARY and ALL are not offered) */
enum { KS_EPS_LARGEST_MAGNITUDE = 1, KS_EPS_SMALLEST_MAGNITUDE = 2, KS_EPS_LARGEST_REAL = 3, KS_EPS_SMALLEST_REAL = 4,
       KS_EPS_LARGEST_IMAGINARY = 5, KS_EPS_SMALLEST_IMAGINARY = 6, KS_EPS_TARGET_MAGNITUDE = 7, KS_EPS_TARGET_REAL = 8,
       KS_EPS_WHICH_USER = 11 };
/* SlepcEigenvalueComparisonFn (include/slepcsc.h): *res < 0 if a is preferred to b, > 0 if b is preferred, 0 if equal */
typedef int (*ks_eig_compare_fn)(double ar, double ai, double br, double bi, int *res, void *ctx);
enum { KS_EPS_HEP = 1, KS_EPS_GHEP = 2, KS_EPS_NHEP = 3, KS_EPS_GNHEP = 4 };   /* EPSProblemType, slepceps.h */
enum { KS_ST_SHIFT = 0, KS_ST_SINVERT = 1, KS_ST_CAYLEY = 2, KS_ST_PRECOND = 3 };   /* STType "shift", "sinvert", "cayley", "precond" (precond.c: K = A - sigma B is only preconditioned, never solved) */
enum { KS_EPS_KRYLOVSCHUR = 0, KS_EPS_LOBPCG = 1, KS_EPS_GD = 2, KS_EPS_JD = 3 };   /* EPSType "krylovschur", "lobpcg", "gd", "jd" */
enum { KS_EPS_ERROR_ABSOLUTE = 0, KS_EPS_ERROR_RELATIVE = 1, KS_EPS_ERROR_BACKWARD = 2 };   /* EPSErrorType */
enum { KS_EPS_RITZ = 0, KS_EPS_HARMONIC = 1, KS_EPS_HARMONIC_RELATIVE, KS_EPS_HARMONIC_RIGHT, KS_EPS_HARMONIC_LARGEST, KS_EPS_REFINED, KS_EPS_REFINED_HARMONIC };  /* EPSExtraction slepceps.h:94-100; Krylov-Schur offers the first two */
enum { KS_EPS_BALANCE_NONE = 0, KS_EPS_BALANCE_ONESIDE = 1, KS_EPS_BALANCE_TWOSIDE = 2, KS_EPS_BALANCE_USER = 3 };   /* EPSBalance slepceps.h; the two-sided form needs the transposed product (ks_mat_mult_transpose) */
enum { KS_EPS_CONV_ABS = 0, KS_EPS_CONV_REL = 1, KS_EPS_CONV_NORM = 2, KS_EPS_CONV_USER = 3 };   /* EPSConv slepceps.h:153-156 */
/* user callbacks of the solver (slepceps.h EPSConvergenceTestFn, EPSStoppingTestFn, EPSMonitorFn); non-zero return = error */
typedef int (*ks_eps_converged_fn)(ks_eps eps, double eigr, double eigi, double res, double *errest, void *ctx);
typedef int (*ks_eps_stopping_fn)(ks_eps eps, int its, int max_it, int nconv, int nev, int *reason, void *ctx);
/* SlepcArbitrarySelectionFn (slepcsc.h): (eigr, eigi, xr, xi, &rr, &ri, ctx); xr/xi are device vectors of n_local doubles */
typedef int (*ks_eps_arbitrary_fn)(double eigr, double eigi, const double *xr_dev, const double *xi_dev, double *rr, double *ri, void *ctx);
typedef int (*ks_eps_monitor_fn)(ks_eps eps, int its, int nconv, const double *eigr, const double *eigi, const double *errest, int nest, void *ctx);
enum { KS_EPS_CONVERGED_TOL = 1, KS_EPS_CONVERGED_USER = 2, KS_EPS_DIVERGED_ITS = -1, KS_EPS_DIVERGED_BREAKDOWN = -2,
       KS_EPS_DIVERGED_SYMMETRY_LOST = -3, KS_EPS_CONVERGED_ITERATING = 0 };

/* ---- context -------------------------------------------------------------------------------- */
/* stream: a hipStream_t owned by the caller (e.g. torch's current stream) or NULL -> own stream. */
int ks_ctx_create(int device, void *stream, ks_ctx *ctx);
int ks_ctx_destroy(ks_ctx ctx);
int ks_ctx_synchronize(ks_ctx ctx);
/* Test hooks (compiled with -DKSD_TEST_HOOKS, which the in-tree build sets): each makes a test run the path the fast one replaces, to compare bits,
 * or a multi-rank path on one rank. Set BEFORE the objects they affect are created: NO_FUSED_GS is read at ks_bv_create, FORCE_MULTI at
 * ks_comm_init_rccl / ks_comm_set_ops, ONESHOT_SEQ0 (first stamp of the one-shot allreduce) at ks_comm_set_allreduce, NO_DICT_PATTERNS (keep the
 * dictionary layout's 2-byte codes per entry, never its row-pattern form) at matrix assembly; the others per call. */
enum { KS_DEBUG_NO_FUSED_GS = 0, KS_DEBUG_NO_MFMA = 1, KS_DEBUG_NO_SPMV_DOT = 2, KS_DEBUG_FORCE_MULTI = 3, KS_DEBUG_HALO_OVERLAP = 4, KS_DEBUG_ONESHOT_SEQ0 = 5,
       KS_DEBUG_NO_DICT_PATTERNS = 6, KS_DEBUG_NO_RESTART_FUSION = 7 /* the final update of a run's last column, the restart product and the copy as the launches of their own */,
       KS_DEBUG_NO_DICT_PAIRS = 8 /* read at launch: the dictionary product one row per lane also where the matrix has the pair form */,
       KS_DEBUG_NO_STEP_FORWARD = 9 /* read at enqueue: the final update of a Krylov step, the next product and the next dot sweep as the launches of their own */ };
int ks_ctx_set_debug(ks_ctx ctx, int key, long long value);
/* Test hook (KSD_TEST_HOOKS): how often the library decided, on this context since the last reset, that a basis is resident in the Infinity Cache
 * (plain loads) and how often that it streams (nontemporal loads). Every evaluation of that rule counts: one per launch in the dot sweep, the
 * Gram-Schmidt update, the fused restart, the Ritz residual, the block residual and the oblique projection, and one where the forward update asks
 * whether it applies (no launch of its own; not reached when an earlier condition already rules it out). A test reads the counts around a call instead
 * of restating the size rule. plain, streaming: either may be NULL; reset != 0 clears both after reading. */
int ks_ctx_basis_load_counts(ks_ctx ctx, long long *plain, long long *streaming, int reset);
int ks_ctx_sync_count(ks_ctx ctx, long long *count);   /* instrumentation: host waits on the context's stream made by the library so far */
int ks_ctx_device_info(ks_ctx ctx, char *arch, int arch_len, int *num_cu, size_t *mem_total);
/* Which HIP runtime the library's calls are bound to. A process can map TWO copies of libamdhip64 (PyTorch wheels bundle one under the file name
 * libamdhip64.so with the SONAME libamdhip64.so.7: loaded AFTER this library they become a second runtime, loaded BEFORE it the dynamic linker binds
 * this library to that copy). ks_ctx_create refuses a process that maps more than one; a process that gains a second one later is reported here and by
 * one warning on stderr at the first occupancy query that fails. Writes a JSON object: {"hip_runtime_path", "hip_runtime_version",
 * "hip_runtimes_mapped": [paths], "occupancy_query_failures", "occupancy_last_error"}. No context needed; never initialises the GPU. */
int ks_runtime_info(char *json, int len);
/* Diagnosis only: let ks_ctx_create proceed in a process that maps two HIP runtimes (scripts/hip_runtime_probe.py reproduces round 3's failures with it). */
int ks_runtime_allow_multiple(int allow);

/* Row-wise distribution (PetscLayout, bvbasic.c:129-134).  Reductions inside BV ops
   (bvblas.c:218,255; bvlapack.c:50) become an allreduce over all ranks; MatMult exchanges the
   boundary entries of x with the owning ranks (PETSc VecScatter inside MatMult_MPIAIJ).
   Two providers: native RCCL over xGMI (ks_comm_init_rccl) or three caller-supplied operations
   (ks_comm_set_ops; e.g. GPU-aware MPI: MPIU_Allreduce / MPI_Allgather / MPI_Isend+Irecv).      */
#define KS_UNIQUE_ID_BYTES 128
int ks_comm_get_unique_id(unsigned char id[KS_UNIQUE_ID_BYTES]);                       /* rank 0, then broadcast by the launcher */
int ks_comm_init_rccl(ks_ctx ctx, int rank, int size, const unsigned char id[KS_UNIQUE_ID_BYTES]);
typedef struct ks_comm_ops {
  /* in-place SUM of `count` doubles in DEVICE memory, ordered on `stream` */
  int (*allreduce_sum)(void *user, double *dev_buf, int count, void *stream);
  /* setup only: every rank contributes `bytes` HOST bytes; recv gets size*bytes, in rank order */
  int (*allgather_host)(void *user, const void *send, int bytes, void *recv);
  /* neighbour exchange on DEVICE buffers, ordered on `stream`: to/from peers[i], segments
     [off[i], off[i]+cnt[i]) in units of elem_bytes */
  int (*exchange)(void *user, int npeers, const int *peers, const void *dev_send, const int *send_off, const int *send_cnt,
                  void *dev_recv, const int *recv_off, const int *recv_cnt, int elem_bytes, void *stream);
} ks_comm_ops;
int ks_comm_set_ops(ks_ctx ctx, int rank, int size, const ks_comm_ops *ops, void *user);
int ks_comm_rank_size(ks_ctx ctx, int *rank, int *size);
/* Known-answer run of the installed communicator: an allreduce with a closed-form sum, two allgathers of one int per rank and
 * a ring exchange with ranks rank+1 / rank-1. Collective; returns KS_ERR_LIB with a message naming the first mismatch. A no-op
 * on a single rank without forced collectives. (The reference leans on MPI's own correctness here; a communicator handed in
 * through ks_comm_set_ops is foreign code, so the library offers the check an integrator runs once after installing it.) */
int ks_comm_check(ks_ctx ctx);
/* Host wall time spent so far in the broadcast of rank 0's projected problem (one per restart with KS_DS_PARALLEL_SYNCHRONIZED, the DSSynchronize analogue,
   dshep.c:673-713): number of broadcasts and their seconds (upload, ncclBroadcast or the provider's allgather, download, host wait); reset != 0 clears them. */
int ks_comm_bcast_stats(ks_ctx ctx, long long *calls, double *seconds, int reset);
/* Which allreduce the Gram-Schmidt passes use. KS_ALLREDUCE_PROVIDER: the communicator's own (ncclAllReduce with the
 * RCCL provider; what bvblas.c:255 MPIU_Allreduce is to the reference). KS_ALLREDUCE_ONESHOT: one kernel per rank writes the k+1
 * values into a mailbox of every rank (peer-mapped uncached device memory: hipIpc between processes, xGMI between GPUs) and adds
 * what arrived in rank order - identical bits on all ranks, no library call on the critical path; reductions longer than 128
 * doubles keep going through the provider. Collective; *active returns what was installed: the one-shot path is taken only if
 * every rank could map every mailbox, else all ranks stay on the provider. A rank that receives no packet within
 * KSGPU_ONESHOT_TIMEOUT_MS (default 2000) returns NaN and the next host wait fails with KS_ERR_LIB - never a hang. */
#define KS_ALLREDUCE_PROVIDER 0
#define KS_ALLREDUCE_ONESHOT 1
int ks_comm_set_allreduce(ks_ctx ctx, int kind, int *active);
int ks_comm_get_allreduce(ks_ctx ctx, int *active);
/* in-place SUM over the ranks of `count` doubles in device memory, ordered on the context's stream (bvblas.c:255 MPIU_Allreduce): the
 * reduction every library kernel uses, for callers that keep their own replicated device scalars (an adapter's VecDot) */
int ks_comm_allreduce_sum(ks_ctx ctx, double *dev_buf, int count);
/* device<->host copy on the context's stream (synchronous); kind: 0 = host->device, 1 = device->host */
int ks_ctx_memcpy(ks_ctx ctx, void *dst, const void *src, size_t bytes, int kind);
/* the same on a given stream (the `stream` argument a ks_comm_ops callback receives; NULL = the context's): what a provider that
   stages through the host uses to order itself after the work already enqueued there */
int ks_ctx_memcpy_stream(ks_ctx ctx, void *dst, const void *src, size_t bytes, int kind, void *stream);
/* fill device memory on the context's stream; enqueues only (what BV_CleanCoefficients_HIP's hipMemset, bvhip.hip.cpp:345-360, is on the
   stream PETSc works on) */
int ks_ctx_memset(ks_ctx ctx, void *dev, int value, size_t bytes);

/* ---- Mat: the MatMult(AIJ) slot ------------------------------------------------------------- */
/* CSR arrays as in PETSc SeqAIJ (i,j,a): rowptr[n_local+1], col[nnz] (GLOBAL column indices),
   val[nnz].  Host arrays are copied to the device.  row_start = first global row owned by this
   rank; n_global = global size.  With one rank: row_start=0, n_local=n_global.               */
int ks_mat_create_csr(ks_ctx ctx, int n_local, int row_start, int n_global,
                      const int *rowptr, const int *col, const double *val, ks_mat *A);
/* The same with options. KS_MAT_KEEP_CSR: the matrix keeps a host copy of the arrays it was created from, as a PETSc AIJ Mat keeps its
   own - what MatDuplicate / MatAXPY need later (ks_mat_create_axpy, ST_MATMODE_COPY); without it only the layout the product runs on
   survives the assembly. Matrices read by ks_mat_load_petsc_binary keep theirs.
   KS_MAT_SHARDED_TRANSPOSE: a row-sharded matrix (more than one rank) gets a transposed product: ks_mat_mult_transpose and
   ks_mat_create_transpose work on it instead of returning KS_ERR_SUP. Needs KS_MAT_KEEP_CSR (KS_ERR_ARG_INCOMP without it); the matrix also keeps
   its ghost list and pack list on the host, and the plan and its device buffers are built at the first transposed product. On one rank the
   flag changes nothing. Without it nothing changes on any number of ranks. */
#define KS_MAT_KEEP_CSR 1u
#define KS_MAT_SHARDED_TRANSPOSE 2u
int ks_mat_create_csr_flags(ks_ctx ctx, int n_local, int row_start, int n_global,
                            const int *rowptr, const int *col, const double *val, unsigned flags, ks_mat *A);
/* P = A + alpha B as a new matrix: MatDuplicate(A,MAT_COPY_VALUES,&P) + MatAXPY(P,alpha,B,DIFFERENT_NONZERO_PATTERN), B == NULL:
   MatShift(P,alpha) - the assembly of A - sigma B in ST_MATMODE_COPY (src/sys/classes/st/interface/stsolve.c:611-626). Entry by
   entry p_ij = a_ij + (alpha b_ij); rows with ascending columns come out ascending. A and B must hold their CSR arrays
   (KS_MAT_KEEP_CSR; KS_ERR_ORDER otherwise) and the same row block. flags as above, for P; when every operand was created with
   KS_MAT_SHARDED_TRANSPOSE (more than one rank), P gets that flag and KS_MAT_KEEP_CSR whatever flags says. */
int ks_mat_create_axpy(ks_mat A, double alpha, ks_mat B, unsigned flags, ks_mat *P);
/* Synthetic generators that build the SAME CSR arrays directly in device memory (bench inputs):
   3-D 7-pt Laplacian of ex19.c:47-78 (rows of z-planes [z0,z0+nz_local) of an nx*ny*nz grid) and
   2-D 5-pt Laplacian of ex2.c:44-51.                                                           */
int ks_mat_create_laplacian3d(ks_ctx ctx, int nx, int ny, int nz, int z0, int nz_local, ks_mat *A);
int ks_mat_create_laplacian2d(ks_ctx ctx, int n, int m, ks_mat *A);
/* MatLoad from a PETSc binary viewer file (the .petsc files under share/slepc/datafiles/matrices, as ex4.c and ex7.c read them); every
   rank takes the row block PETSC_DECIDE would give it */
int ks_mat_load_petsc_binary(ks_ctx ctx, const char *path, ks_mat *A);
/* MatCreateShell + MATOP_MULT (the matrix-free route of src/eps/tutorials/ex3.c): y = mult(user, x) on device
   pointers of n_local doubles; the callback must order its work after everything already enqueued on the context's
   stream (enqueue on that stream, or synchronise) and leave y complete in that order.          */
typedef int (*ks_shell_mult_fn)(void *user, const double *x_dev, double *y_dev);
int ks_mat_create_shell(ks_ctx ctx, int n_local, int row_start, int n_global, ks_shell_mult_fn mult, void *user, ks_mat *A);
int ks_mat_norm_inf(ks_mat A, double *val);                             /* MatNorm(A,NORM_INFINITY) */
int ks_mat_get_diagonal(ks_mat A, double *d_dev);                      /* MatGetDiagonal (local diagonal block) */
int ks_mat_shell_set_enqueue_only(ks_mat A, int flag);   /* the callback only enqueues work on the context's stream: Krylov runs are then enqueued ahead through it */
int ks_mat_destroy(ks_mat A);
int ks_mat_get_sizes(ks_mat A, int *n_local, int *n_global, long long *nnz_local);
/* device layout chosen at assembly for the local diagonal block (KSGPU_SPMV=csr|csrvec|csrregs|sell|dict|odict|binned|sliced|window overrides the choice, any other value fails the creation): dictionary forms for
   stencil-like matrices with few distinct values / offsets, SELL-64 for short regular rows, CSR row blocks for ragged ones, BINNED (two streaming phases, every
   random access in LDS) for matrices whose columns scatter over a vector much larger than an L2; SLICED is round 1's layout for those.
   WINDOW is CSR for ragged rows of more than 16 entries whose columns are stripe-local (mesh orderings with several unknowns per node): rows are cut
   into blocks, a block whose entries reference at most max_segments 64-double segments of x keeps a 16-bit code per entry (10 bytes per nonzero
   instead of 12) and the product stages those segments in LDS and gathers from there; a block that references more keeps its 32-bit columns and
   gathers from memory. Values, row pointers, entry order and the bits of y are those of CSR. Built only when asked for: KSGPU_SPMV=window
   builds it for any matrix with rows and entries; no automatic rule picks it yet. */
enum { KS_MAT_LAYOUT_CSR = 0, KS_MAT_LAYOUT_SELL = 1, KS_MAT_LAYOUT_SLICED = 2, KS_MAT_LAYOUT_SHELL = 3, KS_MAT_LAYOUT_DICT = 4, KS_MAT_LAYOUT_ODICT = 5, KS_MAT_LAYOUT_BINNED = 6,
       KS_MAT_LAYOUT_WINDOW = 7, KS_MAT_LAYOUT_BSR = 8 };
int ks_mat_get_layout(ks_mat A, int *layout);
/* The windowed CSR layout (KS_MAT_LAYOUT_WINDOW). *block_rows (rows of a block) and *max_segments (segments of x a window holds) are the library's two
   constants and are returned for any matrix. For a matrix in this layout: *blocks, *direct_blocks (blocks that reference more segments than a window
   holds), *window_entries (entries of the other blocks) and *index_bytes, the column information a product reads: 2 bytes per window entry, 4 per
   direct entry, 4 per listed segment. Any other layout: these four 0. */
int ks_mat_get_window_info(ks_mat A, int *block_rows, int *max_segments, long long *blocks, long long *direct_blocks, long long *window_entries, long long *index_bytes);
/* MatCreateSeqBAIJWithArrays / MatCreateMPIBAIJWithArrays: a matrix of dense bs x bs blocks. browptr[n_local / bs + 1], bcol[nnzb] (GLOBAL block
   columns; inside a block row in any order, repeats allowed), bval[nnzb bs bs] with block k column-major at bval + k bs bs, as in PETSc's
   Mat_SeqBAIJ::a. The matrix is, in every respect but the device layout of its diagonal block, ks_mat_create_csr_flags of its EXPANSION: scalar row
   bs I + i holds, for each block k of block row I in stored order and then c = 0 .. bs - 1, the entry (bs bcol[k] + c, blk_k(i, c)); explicit zeros
   inside blocks are entries. flags as there (KS_MAT_KEEP_CSR keeps the expanded arrays, so ks_mat_create_axpy, both transposes and every PC
   set-up work unchanged); ks_mat_get_diagonal, ks_mat_norm_inf and ks_mat_get_sizes answer for the expansion.
   Device layout: 2 <= bs <= 8 and KSGPU_SPMV unset: KS_MAT_LAYOUT_BSR - the values at 8 bytes per stored scalar, one int per block, one int per
   block row, no per-entry index: 8 + 4 / bs^2 bytes per scalar against the CSR stream's 12, and one gather of bs contiguous doubles of x per block.
   y = A x and every column of ks_mat_mult_multi are bit for bit what the CSR kernels give on the expansion. bs == 1 or bs > 8: the expansion goes
   through the ordinary chooser; KSGPU_SPMV=<name> forces that layout on the expansion. Matrices from the other creation calls never get this layout,
   nor do ks_mat_create_axpy results and transposes of such a matrix. More than one rank: n_local, row_start and n_global are multiples of bs.
   Errors: bs < 1: KS_ERR_ARG_OUTOFRANGE; a size that is not a multiple of bs: KS_ERR_ARG_SIZ (before any collective); browptr[I + 1] < browptr[I]:
   KS_ERR_ARG_WRONG, and a block column outside [0, n_global / bs): KS_ERR_ARG_OUTOFRANGE, both naming the block row (all row pointers are checked
   before the first block column); more than 2^31 - 1 stored scalars: KS_ERR_ARG_OUTOFRANGE; a failed allocation: KS_ERR_MEM, nothing left half-built. */
int ks_mat_create_bsr(ks_ctx ctx, int bs, int n_local, int row_start, int n_global, const int *browptr, const int *bcol, const double *bval,
                      unsigned flags, ks_mat *A);
/* The block CSR layout (KS_MAT_LAYOUT_BSR): *bs, the library's two constants for that bs - *group_block_rows, the block rows a workgroup takes per
   step, and *chunk_entries, the stored scalars one staging step of a wave brings in - *block_rows and *blocks of the local diagonal block, and
   *index_bytes = 4 blocks + 4 (block_rows + 1), all the index information a product reads. Any other layout: all outputs 0. */
int ks_mat_get_bsr_info(ks_mat A, int *bs, int *group_block_rows, int *chunk_entries, long long *block_rows, long long *blocks, long long *index_bytes);
/* The dictionary layout (KS_MAT_LAYOUT_DICT) stores a row as W 2-byte codes (W = 8, 16 or 32 entry slots). When the matrix has at most 256 distinct
   rows of codes it keeps one byte per row instead, the index of the row's code word in a table of *npatterns words (the row-pattern form), and frees the
   codes. *patterns = 1 in that form, 0 otherwise; *npatterns = 0 and *index_bytes = 2 W n with the codes, n (plus padding to 256 rows) with the
   patterns: the device memory held per row of the diagonal block. Any other layout: all four 0. */
int ks_mat_get_dict_info(ks_mat A, int *patterns, int *npatterns, int *w, long long *index_bytes);
/* the pair form of the row-pattern form (two rows per lane, 16-byte loads of x): whether the matrix has it, its bases, and how many products (the fused dot sweep included) ran in either form */
int ks_mat_get_dict_pairs_info(ks_mat A, int *eligible, int *nbases, long long *pair_launches, long long *row_launches);
/* MatMult: y = A x on device pointers (x, y: n_local doubles owned by this rank).
   Multi-rank: performs the halo exchange of x (PETSc VecScatter inside MatMult_MPIAIJ).        */
int ks_mat_mult(ks_mat A, const double *x_dev, double *y_dev);
/* MatMultTranspose: y = A^T x. An assembled matrix builds its transpose on first use (MatTranspose on the host from the kept CSR arrays:
   KS_MAT_KEEP_CSR, KS_ERR_ORDER otherwise; one rank - the transpose of a row-sharded matrix is a redistribution, KS_ERR_SUP) and multiplies
   with it like any other matrix; a shell matrix needs ks_mat_shell_set_mult_transpose (MATOP_MULT_TRANSPOSE, as ex9.c:123 sets it).
   A row-sharded matrix created with KS_MAT_SHARDED_TRANSPOSE has the product without a redistribution (MatMultTranspose_MPIAIJ): the transposed
   off-diagonal block times the local x into a ghost-length buffer, the transposed diagonal block (its own device layout) times x into y, and
   the forward halo run in reverse - always through the communicator's exchange, also when KS_HALO_PEER is active - after which every listed
   row adds what the other ranks sent. Summation order of an entry of y, fixed: first the diagonal block's sum, in its layout's order, then the
   contributions of the other ranks in ascending rank. No atomics: the same bits on every run. Enqueued, no host wait of the library's own.
   Used by the two-sided balancing (EPSBuildBalance_Krylov epsdefault.c:402-411). */
int ks_mat_mult_transpose(ks_mat A, const double *x_dev, double *y_dev);
int ks_mat_shell_set_mult_transpose(ks_mat A, ks_shell_mult_fn mult_transpose);
/* MatCreateTranspose: *At is a matrix whose ks_mat_mult is ks_mat_mult_transpose(A) and whose transposed product is ks_mat_mult(A); what the
   two-sided solver expands its left basis with. Assembled A: the view is the transposed matrix A builds once for ks_mat_mult_transpose (same
   conditions: KS_MAT_KEEP_CSR or KS_ERR_ORDER, one rank or KS_ERR_SUP), an assembled matrix in its own device layout - Krylov runs are enqueued
   ahead through it and ks_mat_mult on it is bit for bit ks_mat_mult_transpose(A). Shell A: a shell over the transposed callback (KS_ERR_SUP
   without one) with the same enqueue-only flag. The view does not own A and A does not wait for it: destroy the view (ks_mat_destroy) before
   A; destroying A first and using or destroying the view afterwards is the caller's error.
   Row-sharded A created with KS_MAT_SHARDED_TRANSPOSE: the view is the transposed diagonal block with the plan of the reverse exchange; its
   ks_mat_mult is ks_mat_mult_transpose(A) as described there, ks_mat_get_layout reports the transposed diagonal block's layout,
   ks_mat_get_diagonal answers with A's diagonal, ks_mat_mult_multi goes column by column, ks_mat_norm_inf returns KS_ERR_SUP (it would be a
   1-norm of A across ranks). Not collective: the plan is built from what the rank holds. */
int ks_mat_create_transpose(ks_mat A, ks_mat *At);
int ks_mat_mult_host(ks_mat A, const double *x_host, double *y_host);  /* convenience for tests (single rank) */
/* MatMatMult / MatProductNumeric(AB) with a dense column-major block: Y(:,j) = A X(:,j), j < ncols (X(:,j) at X_dev + j*ldx, Y(:,j) at
   Y_dev + j*ldy). Every column is bit for bit ks_mat_mult(A, X(:,j)): the dictionary, offset-dictionary, SELL-64 and CSR row-block layouts
   apply A to up to 8 columns per pass (the matrix streamed once per pass); BINNED, SLICED, WINDOW, shell matrices, the CSR-vector form of small
   matrices and row-sharded matrices with a halo run one ks_mat_mult per column. ncols == 0 does nothing; ldx, ldy >= max(1, n_local)
   (KS_ERR_ARG_SIZ); X and Y must not overlap (KS_ERR_ARG_WRONG). Enqueued on the context's stream, no host wait. */
int ks_mat_mult_multi(ks_mat A, int ncols, const double *X_dev, int ldx, double *Y_dev, int ldy);
/* How MatMult moves the boundary entries of x between ranks. KS_HALO_PROVIDER: packed into a send buffer and handed to the
 * communicator's exchange (grouped ncclSend / ncclRecv with the RCCL provider; PETSc's VecScatter is the reference's). KS_HALO_PEER: the pack
 * kernel stores every boundary entry straight into the ghost mailbox of the rank that needs it (device memory of that rank mapped here:
 * hipIpc between processes, xGMI between GPUs), stamped and acknowledged per product, and the receiver copies its mailbox into its ghost
 * array - no library call per product. Collective; *active returns what was installed: the peer path only if every rank could map all
 * its neighbours' mailboxes (at most 16 neighbours per rank). A rank that waits longer than KSGPU_ONESHOT_TIMEOUT_MS (default 2000) for a
 * neighbour fills its ghosts with NaN and the next host wait fails with KS_ERR_LIB - never a hang.
 * Taking the peer path down is collective too: ks_mat_set_halo(A, KS_HALO_PROVIDER) (or a new KS_HALO_PEER set-up) lets every rank finish, closes the
 * mapped mailboxes and only then frees its own. Call it before ks_mat_destroy on a matrix whose peer halo is active; a destroy without it waits (bounded)
 * for the neighbours' last acknowledgements before freeing the mailbox, but cannot wait for them to unmap it. */
#define KS_HALO_PROVIDER 0
#define KS_HALO_PEER 1
int ks_mat_set_halo(ks_mat A, int kind, int *active);
int ks_mat_get_halo(ks_mat A, int *active);

/* ---- BV: the _BVOps slots ------------------------------------------------------------------- */
int ks_bv_create(ks_ctx ctx, int n_local, int n_global, int m, int ld /*0: default*/, ks_bv *bv); /* ops->create, BV_SetDefaultLD bvimpl.h:471 */
int ks_bv_destroy(ks_bv bv);                                                        /* ops->destroy */
int ks_bv_duplicate(ks_bv bv, ks_bv *out);                                           /* ops->duplicate (storage only; no copy) */
int ks_bv_get_sizes(ks_bv bv, int *n_local, int *n_global, int *m, int *ld);
int ks_bv_set_ownership_start(ks_bv bv, int row_start);                             /* first global row of this rank (PetscLayout rstart); used by the reproducible random vectors */
int ks_bv_set_active_columns(ks_bv bv, int l, int k);                               /* BVSetActiveColumns bvbasic.c:421 */
int ks_bv_get_active_columns(ks_bv bv, int *l, int *k);
int ks_bv_set_orthogonalization(ks_bv bv, int type, int refine, double eta);        /* BVSetOrthogonalization; eta<=0 keeps 0.7071 */
int ks_bv_get_array(ks_bv bv, double **dev);                                        /* ops->getarray: device pointer of the m*ld block */
int ks_bv_get_column(ks_bv bv, int j, double **dev);                                /* ops->getcolumn: device pointer view of column j (j<0: constraint) */
int ks_bv_get_buffer(ks_bv bv, double **dev);                                       /* BVGetBufferVec bvbasic.c:775: (nc+m)*m device doubles */
int ks_bv_set_buffer(ks_bv bv, double *dev);                                        /* BVSetBufferVec bvbasic.c:720 on a raw device array of (nc+m)*m doubles (caller-owned; NULL: the library's own) */
int ks_bv_set_layout(ks_bv bv, int nc, int m);                                      /* mirror of the fields BVSetNumConstraints changes (bvbasic.c:291-296); moves no data */
int ks_bv_set_column_host(ks_bv bv, int j, const double *host);                     /* H2D of n_local doubles */
int ks_bv_get_column_host(ks_bv bv, int j, double *host);                           /* D2H, synchronises */
int ks_bv_get_buffer_host(ks_bv bv, double *host);                                  /* D2H of the (nc+m)*m coefficient buffer */
int ks_bv_resize(ks_bv bv, int m, int copy);                                    /* BVResize bvbasic.c:190 (ops->resize) */
int ks_bv_set_random(ks_bv bv, uint64_t seed);                                   /* BVSetRandom bvops.c:380: all active columns */
int ks_bv_insert_vec(ks_bv bv, int j, const double *w_dev);                      /* BVInsertVec bvops.c:568 */
int ks_bv_copy_vec(ks_bv bv, int j, double *w_dev);                              /* BVCopyVec bvops.c:484 */
int ks_bv_insert_vecs(ks_bv bv, int s, int *m, const double *const *W_dev, int orth); /* BVInsertVecs bvfunc.c:331: *m device vectors into columns s..; orth drops dependent ones, *m = kept */
int ks_bv_insert_constraints(ks_bv bv, int *nc, const double *const *C_dev);     /* BVInsertConstraints bvfunc.c:411: destructive; *nc = kept; constraints are columns -nc..-1 */
int ks_bv_set_num_constraints(ks_bv bv, int nc);                                 /* BVSetNumConstraints bvbasic.c:260 */
int ks_bv_get_num_constraints(ks_bv bv, int *nc);                                /* BVGetNumConstraints bvbasic.c:310 */
int ks_bv_set_random_column(ks_bv bv, int j, uint64_t seed);                        /* BVSetRandomColumn with -bv_reproducible_random semantics */

int ks_bv_mult(ks_bv Y, double alpha, double beta, ks_bv X, const double *Q, int ldq);          /* ops->mult; Q NULL -> Y=beta*Y+alpha*X */
int ks_bv_multvec(ks_bv X, double alpha, double beta, double *y_dev, const double *q);          /* ops->multvec; q NULL -> buffer */
int ks_bv_multcolumn(ks_bv X, double alpha, double beta, int j, const double *q);               /* BVMultColumn bvops.c:165 */
int ks_bv_multinplace(ks_bv V, const double *Q, int ldq, int s, int e);                          /* ops->multinplace */
int ks_bv_multinplace_trans(ks_bv V, const double *Q, int ldq, int s, int e);                    /* ops->multinplacetrans */
/* The end of a restart cycle: BVMultInPlace(V,Q,s,e) followed by BVCopyColumn(V,src,dst). With ks_bv_set_defer_final on, a Krylov run
   (ks_bv_matlanczos / ks_bv_matarnoldi) keeps the final Gram-Schmidt update of its last column back; this call then applies it inside the
   product's sweep: one launch and one read of the panel for update, product and copy. Every other entry point that reads or writes
   column data or Gram-Schmidt state applies a waiting update first, so the deferral is never visible in results: memory and coefficients are
   bit for bit what the separate launches leave. One rank, at most 32 columns before src, at most 16 product columns; other shapes run the
   separate launches. ks_bv_restart_stats: whether an update is waiting, how many were applied on their own, how many inside a restart. */
int ks_bv_restart(ks_bv V, const double *Q, int ldq, int s, int e, int src, int dst);
int ks_bv_set_defer_final(ks_bv bv, int on);
int ks_bv_restart_stats(ks_bv bv, int *pending, long long *flushes, long long *fused);
/* Forward form of the final update (an enqueued Krylov run on one rank, pair-form dictionary matrix of at most five bases, basis streaming from HBM):
   the launch that stores column j + 1 also forms y = A v_{j+1} and the first dots of the next step; the ordinary product and dot sweep stay enqueued
   behind it and run only if the device did not take the form (a column that left the two-pass program) or a bounded wait inside it gave up.
   ks_bv_step_forward_stats (waits for the stream): launches whose bookkeeping took the form, those that completed, those that gave up, fallback
   products that ran. ks_bv_step_forward_info: forward launches enqueued so far and why the last column asked about was refused ("" if it was not).
   Test hooks (KSD_TEST_HOOKS) ks_bv_step_forward_hooks: force != 0 drops the size conditions (16 tiles per CU, basis not cache-resident); grid > 0
   forces the number of workgroups; budget >= 0 replaces the wall-time budget of a wait (ticks of 10 ns; 0: every wait gives up);
   abort_wg >= 0 makes that workgroup give up at its first wait; lag_odd != 0 makes odd workgroups sleep before they publish a tile. */
int ks_bv_step_forward_stats(ks_bv bv, long long *taken, long long *completed, long long *aborted, long long *fell_back);
int ks_bv_step_forward_info(ks_bv bv, long long *enqueued, char *why, int why_len);
int ks_bv_step_forward_hooks(ks_bv bv, int force, int grid, long long budget, int abort_wg, int lag_odd);
int ks_bv_dot(ks_bv X, ks_bv Y, double *M, int ldm);                                             /* ops->dot: M = Y^H X (+allreduce) */
int ks_bv_dotvec(ks_bv X, const double *y_dev, double *m);                                       /* ops->dotvec; m NULL -> buffer */
int ks_bv_dotvec_local(ks_bv X, const double *y_dev, double *m);                                 /* ops->dotvec_local (no reduction) */
int ks_bv_dotcolumn(ks_bv X, int j, double *q);                                                  /* BVDotColumn bvglobal.c:302 */
/* split reductions (bvglobal.c:207-300, 343-430, 573-660, 705-790): the Begin calls queue this rank's parts on the device, the first
   End reduces everything queued with ONE allreduce; Ends in the order of the Begins. Norms: 2-norm (or the B-norm) only. */
int ks_bv_dotvec_begin(ks_bv X, const double *y_dev, double *m);       int ks_bv_dotvec_end(ks_bv X, const double *y_dev, double *m);
int ks_bv_dotcolumn_begin(ks_bv X, int j, double *q);                  int ks_bv_dotcolumn_end(ks_bv X, int j, double *q);
int ks_bv_normvec_begin(ks_bv bv, const double *v_dev, int type, double *val);  int ks_bv_normvec_end(ks_bv bv, const double *v_dev, int type, double *val);
int ks_bv_normcolumn_begin(ks_bv bv, int j, int type, double *val);    int ks_bv_normcolumn_end(ks_bv bv, int j, int type, double *val);
int ks_bv_scale(ks_bv bv, double alpha);                                                         /* ops->scale(-1,alpha) */
int ks_bv_scalecolumn(ks_bv bv, int j, double alpha);                                            /* ops->scale(j,alpha) */
int ks_bv_norm(ks_bv bv, int type, double *val);                                                 /* ops->norm(-1,type) */
int ks_bv_normcolumn(ks_bv bv, int j, int type, double *val);                                    /* ops->norm(j,type) */
int ks_bv_norm_local(ks_bv bv, int j, int type, double *val);                                    /* ops->norm_local */
int ks_bv_normvec(ks_bv bv, const double *v_dev, int type, double *val);                         /* BVNormVec bvglobal.c:530: norm of a device vector, B-norm when a matrix is set */
int ks_bv_copy(ks_bv V, ks_bv W);                                                                /* ops->copy */
int ks_bv_copycolumn(ks_bv V, int j, int i);                                                     /* ops->copycolumn */
int ks_bv_matmult(ks_bv V, ks_mat A, ks_bv W);                                                   /* ops->matmult (column loop, svec.c:213) */
int ks_bv_matmultcolumn(ks_bv V, ks_mat A, int j);                                               /* BVMatMultColumn bvops.c:862 */
/* BVSetMatMultMethod bvbasic.c:1020 (BVMatMultType slepcbv.h:106-108): how ks_bv_matmult (V's method), ks_bv_matproject and the B*X block
   of ks_bv_dot with an inner-product matrix (X's method) apply a matrix to a block of columns. VECS: one ks_mat_mult per column; MAT:
   one ks_mat_mult_multi (same bits). MAT_SAVE is stored as MAT (bvbasic.c:1053-1055); any other value is KS_ERR_ARG_OUTOFRANGE. The
   default stays VECS (SLEPc's is MAT: INTEGRATION.md section 2); ks_bv_duplicate copies the method. */
enum { KS_BV_MATMULT_VECS = 0, KS_BV_MATMULT_MAT = 1, KS_BV_MATMULT_MAT_SAVE = 2 };
int ks_bv_set_matmult_method(ks_bv bv, int method);
int ks_bv_get_matmult_method(ks_bv bv, int *method);                                             /* BVGetMatMultMethod bvbasic.c:1064 */
/* The residual block of a block eigensolver with its norms (what lobpcg.c:176-202 does with BVCopy, one VecAXPY and one VecNorm per column - bs host
   waits): R(:,j) = AX(:,j) - theta[j - l] * BX(:,j) for the active columns [l, k) of R, at most 16, the same column indices in AX and BX, and
   norms[j - l] = ||R(:,j)||_2 over all ranks (host array). One kernel reads the two blocks once and writes the third, one reduction and one D2H bring
   all the norms. r = fma(-theta, bx, ax): one rounding where the reference has two. BX may be the BV of the vectors themselves (a standard problem);
   R must be a BV of its own (KS_ERR_ARG_WRONG). Columns of R outside [l, k) are not touched. theta: host array. */
int ks_bv_block_residual(ks_bv R, ks_bv AX, ks_bv BX, const double *theta, double *norms);
/* The Ritz vectors of a Davidson iteration with their residuals (what dvd_calcpairs_res_0, dvdcalcpairs.c:523-560, does with two or three BVMult, a
   BVMultVec and two VecNorm per pair): one sweep over the search basis and its images.
   For j < ncols, m = k - l the active columns [l,k) of V, the same column indices in AV and BV:
     x_j  = sum_c V (:, l+c) S(c,j)          (never stored)
     ax_j = sum_c AV(:, l+c) S(c,j)
     bx_j = sum_c BV(:, l+c) S(c,j)          (BV == NULL: a standard problem, bx_j = x_j)
     R(:, lR + j) = ax_j - theta[j] * bx_j,   lR = first active column of R
     rnorm[j] = ||R(:, lR+j)||_2,  xnorm[j] = ||x_j||_2   over all ranks (host arrays; xnorm may be NULL)
   S: host, column-major, m x ncols, lds >= m (staged on the device by the call).  theta: host.
   Every sum starts at 0 and takes c in ascending order with one fma per term, r = fma(-theta, bx, ax): an entry of R depends on its own row alone,
   its bits do not change with the grid, the alignment of the columns or the way the rows are cut over ranks. With a BV, more than 8 result columns
   run as two passes over the panels inside the call (the register budget of a pass: 8 columns generalized, 16 standard). One reduction, one allreduce and one D2H bring all 2 ncols norms. Columns of R outside [lR, lR + ncols) are
   not touched. Errors: ncols outside 1..16, or no active column in V: KS_ERR_ARG_OUTOFRANGE; lds < m, AV / BV with fewer than k columns, R with
   fewer than lR + ncols: KS_ERR_ARG_SIZ; R the same BV as V, AV or BV: KS_ERR_ARG_WRONG; different local sizes: KS_ERR_ARG_INCOMP. */
int ks_bv_ritz_residual(ks_bv R, ks_bv V, ks_bv AV, ks_bv BV, const double *S, int lds, int ncols, const double *theta, double *rnorm, double *xnorm);
/* The same sweep, which also keeps what it has in registers (dvd_improvex_jd_start, dvdimprovex.c, needs the Ritz vectors of the block and their
   images under B as columns): X(:, lX + j) = x_j and BX(:, lBX + j) = bx_j (x_j again without BV), each from the first active column of its BV,
   each optional (NULL). R, rnorm and xnorm have the bits of ks_bv_ritz_residual on the same inputs. Further errors: X or BX the same BV as another
   argument: KS_ERR_ARG_WRONG; fewer than ncols columns from its first active one: KS_ERR_ARG_SIZ; another local size: KS_ERR_ARG_INCOMP. */
int ks_bv_ritz_residual_vectors(ks_bv R, ks_bv V, ks_bv AV, ks_bv BV, const double *S, int lds, int ncols, const double *theta, double *rnorm, double *xnorm, ks_bv X, ks_bv BX);
/* The oblique projector of the Jacobi-Davidson correction equation (dvd_improvex_apply_proj, dvdimprovex.c:220-280, applied to the vector the
   operator has just produced), fused with the linear combination that forms that vector:
     t_i = a * u_i;  if (v) t_i += b * v_i;  w_i = s ? s_i * t_i : t_i          (the rounding of the ST's own combinations)
     h = Z^T w,  c = Minv h,   Z and Y: the k active columns of the two BVs, Minv: k x k on the DEVICE, column-major, ldm >= k
     w_i <- w_i - sum_j Y(i,j) c_j,  j ascending, one fma each, starting from w_i
     e given: *dot = e^T w of the result, summed over all ranks (e == w: ||w||^2)
   All vectors are device arrays of the BVs' local size; v, s, e may be NULL; u == w is allowed. The dot sweep forms and stores w in the same pass, a
   one-workgroup kernel reduces h and multiplies by Minv, the sum over the ranks runs on the device buffer of c (nothing on one rank), the update
   sweep reads c from the device: no host wait between them. With dot == NULL the call only enqueues; with a dot the fixed-order sum of the
   update's partial sums is one more launch and the call waits once. k == 0: the combination and the dot only. More than 64 columns: chunks.
   Errors: different local sizes or column counts of Y and Z: KS_ERR_ARG_INCOMP; ldm < k: KS_ERR_ARG_SIZ; w or u NULL (Minv with k > 0; e with a
   dot): KS_ERR_ARG_NULL; w inside the storage of Y or Z: KS_ERR_ARG_WRONG. */
int ks_bv_oblique_project(ks_bv Y, ks_bv Z, const double *Minv_dev, int ldm, double a, const double *u_dev, double b, const double *v_dev,
                          const double *s_dev, double *w_dev, const double *e_dev, double *dot);

/* ops->gramschmidt (bvimpl.h:53): ONE Gram-Schmidt pass, the function BVOrthogonalizeGS1 dispatches to (bvorthog.c:134) in place
   of BVOrthogonalizeCGS1 (:91-132) / BVOrthogonalizeMGS1 (:52-85), chosen by the BV's orthogonalization type. The caller
   (BVOrthogonalizeGS :145-217) owns the refinement loop, lindep, BV_CleanCoefficients and BV_SetValue.
     v_dev NULL : column j against the constraints and columns 0..j-1;  v_dev given: that device vector against columns [-nc, j)
     which      : MGS only, may be NULL
     h, c       : HOST arrays of nc+m entries (bv->h, bv->c), or both NULL = column j and the scratch column of the BV's buffer;
                  the pass ADDS its coefficients to h (BV_AddCoefficients), c holds this pass's coefficients
     onrm, nrm  : norm before the pass / estimated norm after it (explicit when the estimate breaks down); either may be NULL
   Returns KS_ERR_USER_INPUT for an invalid inner product (BV_SafeSqrt).
   Column form, CGS, standard inner product: the pass is ONE dot sweep and ONE update launch; onrm / nrm reach the host while the update
   still runs (the call waits for the pass's bookkeeping, not for the stream). The other forms synchronise.                          */
int ks_bv_gramschmidt_pass(ks_bv bv, int j, double *v_dev, const int *which, double *h, double *c, double *onrm, double *nrm);
/* Pass chaining for the slot above. `state` is the caller's modification counter of the BV - PetscObjectStateGet((PetscObject)bv,&state):
   PETSc bumps it in BVRestoreColumn (when the Vec was written), BVScaleColumn, BVMultInPlace ... (bvbasic.c:1176, bvops.c:356,243), i.e. whenever the contents may have
   changed, and NOT between the passes BVOrthogonalizeGS makes on one column (bvorthog.c:176-202). Once a state has been announced, a pass whose
   bookkeeping predicts that the caller's refinement loop comes back (same policy, same eta: ks_bv_set_orthogonalization) leaves the dot
   products of the next pass behind, and the next ks_bv_gramschmidt_pass on the same column under the SAME state uses them instead of a dot
   sweep: 3 reads of the basis per CGS2 step instead of 4. Any other state, column or intervening sweep of this BV: the pass takes its own
   dots, as before. A caller that never calls this gets the unchained behaviour. The caller promises that the state changes whenever BV storage
   or the coefficient buffer is written by anyone but ks_bv_gramschmidt_pass itself. */
int ks_bv_set_state(ks_bv bv, uint64_t state);
/* instrumentation: passes of the slot that were chained to their predecessor's dots / that ran their own dot sweep */
int ks_bv_gs_chain_stats(ks_bv bv, long long *chained, long long *fresh);
/* The whole of BVOrthogonalizeColumn / BVOrthonormalizeColumn (not ops slots: the entry points a caller uses that drives this
   library directly): fused, device-resident classical Gram-Schmidt of column j against columns [0,j) with the reference's
   refinement policy; coefficients accumulate in the buffer column j.                              */
int ks_bv_orthogonalizecolumn(ks_bv bv, int j, double *H, double *norm, int *lindep);            /* BVOrthogonalizeColumn bvorthog.c:315 */
int ks_bv_orthonormalizecolumn(ks_bv bv, int j, int replace, double *norm, int *lindep);         /* BVOrthonormalizeColumn bvorthog.c:380 */
int ks_bv_orthogonalizevec(ks_bv bv, double *v_dev, double *H, double *norm, int *lindep);       /* BVOrthogonalizeVec bvorthog.c:247 */
/* BVOrthogonalize bvorthog.c:729: QR of the active columns, V0 = V R, leading columns untouched. R (host, column-major,
   ldr >= k) may be NULL; only its columns l..k-1 are written (upper triangular except for SVQB). The block method is the
   fourth argument of BVSetOrthogonalization.                                                                          */
int ks_bv_set_orthog_block(ks_bv bv, int block);
/* BVSetMatrix(bv,B,PETSC_FALSE) bvfunc.c:200: inner products, norms of columns and every orthogonalisation use y^H B x
   (B symmetric positive definite; borrowed; NULL restores the standard inner product) */
int ks_bv_set_matrix(ks_bv bv, ks_mat B);
int ks_bv_get_matrix(ks_bv bv, ks_mat *B);
int ks_bv_orthogonalize(ks_bv V, double *R, int ldr);
int ks_bv_matproject(ks_bv X, ks_mat A /* NULL: identity */, ks_bv Y, double *M, int ldm);   /* BVMatProject bvglobal.c:1014: M = Y^H A X */
int ks_bv_normalize(ks_bv V, const double *eigi /* may be NULL; entry 0 belongs to column l (what the ops->normalize slot receives after svec.c:196's offset) */);   /* BVNormalize bvglobal.c:855 */
int ks_bv_orthogonalizesomecolumn(ks_bv bv, int j, const int *which, double *H, double *norm, int *lindep); /* bvorthog.c:432 (MGS) */
int ks_bv_gs_passes(ks_bv bv, long long *passes_total, int *passes_last);                        /* instrumentation */

/* Krylov expansions (bvkrylov.c).  H: host ldh x >=m column-major; T: host, alpha = T[0..ldt),
   beta = T[ldt..2ldt) (DS_MAT_T layout).  *m may be reduced on breakdown.  The whole run of
   m-k steps is enqueued without host synchronisation; one D2H at the end (the reference's
   VecGetArrayRead(buf), bvkrylov.c:103,215).                                                   */
int ks_bv_matarnoldi(ks_bv V, ks_mat A, double *H, int ldh, int k, int *m, double *beta, int *breakdown);
int ks_bv_matlanczos(ks_bv V, ks_mat A, double *T, int ldt, int k, int *m, double *beta, int *breakdown);

/* ---- EPS: Krylov-Schur driver (host side; restates krylovschur.c:227-337) -------------------- */
int ks_eps_create(ks_ctx ctx, ks_eps *eps);
int ks_eps_destroy(ks_eps eps);
int ks_eps_set_operators(ks_eps eps, ks_mat A, ks_mat B /* NULL: standard problem */);   /* EPSSetOperators epssetup.c:450 */
int ks_eps_set_problem_type(ks_eps eps, int type);                         /* KS_EPS_HEP / KS_EPS_GHEP (Lanczos, B-inner product) | KS_EPS_NHEP / KS_EPS_GNHEP (Arnoldi) */
int ks_eps_set_dimensions(ks_eps eps, int nev, int ncv /*<=0: default*/, int mpd /*<=0: default*/);
int ks_eps_set_tolerances(ks_eps eps, double tol /*<=0: 1e-8*/, int max_it /*<=0: default*/);
int ks_eps_set_which_eigenpairs(ks_eps eps, int which);
int ks_eps_get_st(ks_eps eps, ks_st *st);                                    /* EPSGetST: borrowed, owned by the EPS */
int ks_eps_set_target(ks_eps eps, double target);                            /* EPSSetTarget epsopts.c:604 (sorting only: no spectral transformation) */
int ks_eps_set_eigenvalue_comparison(ks_eps eps, ks_eig_compare_fn fn, void *ctx);   /* EPSSetEigenvalueComparison epsopts.c:563 */
int ks_eps_set_krylovschur_restart(ks_eps eps, double keep);               /* EPSKrylovSchurSetRestart, default 0.5 */
int ks_eps_set_convergence_test(ks_eps eps, int conv);                    /* EPSSetConvergenceTest: KS_EPS_CONV_* (epsdefault.c:224-257) */
int ks_eps_set_krylovschur_locking(ks_eps eps, int lock);               /* EPSKrylovSchurSetLocking: 0 = non-locking variant (krylovschur.c:294) */
int ks_eps_set_random_seed(ks_eps eps, uint64_t seed);
int ks_eps_set_initial_vector(ks_eps eps, const double *v_host);           /* EPSSetInitialSpace with one vector */
int ks_eps_set_initial_space(ks_eps eps, int n, const double *const *v_dev);   /* EPSSetInitialSpace epssetup.c:590: device vectors; a Krylov solver uses the first */
int ks_eps_set_deflation_space(ks_eps eps, int n, const double *const *v_dev); /* EPSSetDeflationSpace epssetup.c:555: n device vectors, copied; used by the next solve only */
/* DSSetParallel on the solver's DS (dsbasic.c; krylovschur.c:281 DSSynchronize): with KS_DS_PARALLEL_SYNCHRONIZED, after every projected
   solve rank 0's projected matrix, vectors, eigenvalues and the outcome of the expansion (beta, length, breakdown) are broadcast, so the
   replicated control flow cannot diverge when a caller-supplied allreduce does not return identical bits on every rank. Default:
   synchronized (the reference's default is redundant). Cost per restart: 2 ld^2 + 2 ncv + 3 doubles from rank 0 - 16 KB at ncv = 30,
   66 KB at ncv = 64 - as one ncclBroadcast and one host wait with the RCCL provider; a caller-supplied provider has no broadcast
   slot and pays an allgather of that many bytes per rank. */
enum { KS_DS_PARALLEL_REDUNDANT = 0, KS_DS_PARALLEL_SYNCHRONIZED = 1 };
int ks_eps_set_ds_parallel(ks_eps eps, int pmode);
int ks_eps_get_ds_parallel(ks_eps eps, int *pmode);
int ks_eps_set_max_steps(ks_eps eps, long long max_steps);                 /* bench harness: stop after this many Arnoldi steps (0 = off) */
int ks_eps_solve(ks_eps eps);
int ks_eps_get_converged(ks_eps eps, int *nconv);
int ks_eps_get_iteration_number(ks_eps eps, int *its);
int ks_eps_get_converged_reason(ks_eps eps, int *reason);
int ks_eps_get_dimensions(ks_eps eps, int *nev, int *ncv, int *mpd);
int ks_eps_get_eigenvalue(ks_eps eps, int i, double *eigr, double *eigi);
int ks_eps_get_eigenvector_host(ks_eps eps, int i, double *xr_host);       /* n_local doubles */
/* EPSGetEigenpair epssolve.c:405: conjugate pairs come as (xr,xi) of the first and (xr,-xi) of the second member
   (BV_GetEigenvector bvimpl.h:423-446); any of the four outputs may be NULL */
int ks_eps_get_eigenpair_host(ks_eps eps, int i, double *eigr, double *eigi, double *xr_host, double *xi_host);
int ks_eps_get_eigenpair(ks_eps eps, int i, double *eigr, double *eigi, double *xr_dev, double *xi_dev);   /* the same into device vectors of n_local doubles */
int ks_eps_get_invariant_subspace(ks_eps eps, double *const *v_dev);        /* EPSGetInvariantSubspace epssolve.c:247: nconv device vectors; non-symmetric: before any eigenvector is asked for */
int ks_eps_get_error_estimate(ks_eps eps, int i, double *errest);
int ks_eps_compute_error(ks_eps eps, int i, int type, double *error);      /* EPSComputeError epssolve.c:742 */
/* getters of the settings (EPSGetTolerances, EPSGetWhichEigenpairs, EPSGetTarget, EPSGetConvergenceTest, EPSGetOperators,
   EPSGetProblemType with EPSIsGeneralized / IsHermitian / IsPositive); any output may be NULL */
int ks_eps_get_tolerances(ks_eps eps, double *tol, int *max_it);
int ks_eps_get_which_eigenpairs(ks_eps eps, int *which);
int ks_eps_get_target(ks_eps eps, double *target);
int ks_eps_get_convergence_test(ks_eps eps, int *conv);
int ks_eps_set_extraction(ks_eps eps, int extr);                          /* EPSSetExtraction epsopts.c:968: KS_EPS_RITZ | KS_EPS_HARMONIC (target = EPSSetTarget) */
int ks_eps_get_extraction(ks_eps eps, int *extr);
int ks_eps_set_convergence_test_function(ks_eps eps, ks_eps_converged_fn fn, void *ctx); /* EPSSetConvergenceTestFunction: selects KS_EPS_CONV_USER; NULL restores the relative test */
int ks_eps_set_stopping_test_function(ks_eps eps, ks_eps_stopping_fn fn, void *ctx);    /* EPSSetStoppingTestFunction (ex29.c); NULL = EPSStoppingBasic */
int ks_eps_stopping_basic(ks_eps eps, int its, int max_it, int nconv, int nev, int *reason, void *ctx); /* EPSStoppingBasic epsdefault.c:290 */
int ks_eps_set_arbitrary_selection(ks_eps eps, ks_eps_arbitrary_fn fn, void *ctx);      /* EPSSetArbitrarySelection epsopts.c:600 (symmetric variant; the DS sorts on rr/ri, krylovschur.c:275-279); NULL disables */
int ks_eps_monitor_set(ks_eps eps, ks_eps_monitor_fn fn, void *ctx);                    /* EPSMonitorSet (one slot; NULL cancels): called once per restart with the DS-ordered values, untransformed */
int ks_eps_set_purify(ks_eps eps, int purify);                              /* EPSSetPurify: 0 skips the purification of GHEP eigenvectors (test1_1_ks_nopurify) */
int ks_eps_get_purify(ks_eps eps, int *purify);
/* EPSSetType (epsbasic.c): KS_EPS_KRYLOVSCHUR (the default: nothing changes for existing callers), KS_EPS_GD (below) or KS_EPS_LOBPCG, the block solver for the smallest
   (or largest) eigenvalues of symmetric problems without inner solves (src/eps/impls/cg/lobpcg/lobpcg.c; ks_lobpcg.hip). Choosing LOBPCG makes
   KS_ST_PRECOND the type of the solver's ST unless the caller set one (EPSSetDefaultST_Precond); a Krylov-Schur solve with KS_ST_PRECOND is KS_ERR_SUP.
   ks_eps_solve with LOBPCG (EPSSetUp_LOBPCG lobpcg.c:55-83) returns
     KS_ERR_SUP         problem type other than KS_EPS_HEP / KS_EPS_GHEP; `which` other than smallest / largest real (unset: smallest real); arbitrary
                        selection, harmonic extraction or the two-sided flag set; n_global - (deflation vectors) < 5 bs
     KS_ERR_USER_INPUT  ncv given and smaller than max(3 bs, ((nev - 1) / bs + 3) bs); mpd given and different from 3 bs
   Balancing is ignored; the default max_it is max(100, 2 n / ncv). Every getter of results, the monitor, the convergence and stopping tests, the
   deflation space, track-all and the random seed work as after a Krylov-Schur solve; ks_eps_set_initial_space, called after the type is set, hands ALL its vectors to the first blocks (with the default type only the first is kept, as before).
   Convergence is tested on the residual norm ||A x - theta B x||_2 with the EPS's criterion. Stated deviations: block sizes 1..16 only (the projected
   problem has at most 48 columns; larger is KS_ERR_ARG_OUTOFRANGE), and those listed at the top of ks_lobpcg.hip. */
int ks_eps_set_type(ks_eps eps, int type);
int ks_eps_get_type(ks_eps eps, int *type);
int ks_eps_lobpcg_set_blocksize(ks_eps eps, int bs);      /* EPSLOBPCGSetBlockSize lobpcg.c:422; 0 = default min(16, nev) */
int ks_eps_lobpcg_get_blocksize(ks_eps eps, int *bs);     /* EPSLOBPCGGetBlockSize (0 until set) */
int ks_eps_lobpcg_set_restart(ks_eps eps, double r);      /* EPSLOBPCGSetRestart lobpcg.c:472: default 0.9, 0.1..1; guard vectors = min((int)((1 - r) bs + 0.45), bs - 1), 0 for bs = 1 */
int ks_eps_lobpcg_get_restart(ks_eps eps, double *r);
int ks_eps_lobpcg_set_locking(ks_eps eps, int lock);      /* EPSLOBPCGSetLocking lobpcg.c:536 (soft locking), default on */
int ks_eps_lobpcg_get_locking(ks_eps eps, int *lock);
/* instrumentation of the last LOBPCG solve: passes of the main loop, hard locks, columns a matrix was applied to (A and B), columns preconditioned */
int ks_eps_lobpcg_get_stats(ks_eps eps, long long *iterations, long long *hard_locks, long long *mat_columns, long long *pc_columns);
/* KS_EPS_GD: Generalized Davidson (src/eps/impls/davidson: davidson.c, dvdinitv.c, dvdcalcpairs.c, dvdimprovex.c, dvdupdatev.c, dvdtestconv.c;
   ks_gd.hip) for KS_EPS_HEP and KS_EPS_GHEP with a B-orthonormal search basis and Ritz extraction. Every iteration multiplies the new basis columns by
   A (and B), solves the projected problem, forms the Ritz vectors and residuals of the best bs pairs (ks_bv_ritz_residual), tests them in order on
   ||r|| / ||x|| with the EPS's criterion, and then locks the converged pairs, or restarts (minv Ritz vectors plus plusk vectors of the previous
   iteration), or expands the basis by the preconditioned residuals D = M^-1 R. Choosing GD makes KS_ST_PRECOND the type of the solver's ST unless the
   caller set one; the preconditioner is built on A - sigma B with sigma the ST's shift if set, else the target for the target criteria, else 0; for the
   largest-* criteria with no shift set the default shift is infinite (davidson.c:80): M is built on B alone, and a standard problem is not preconditioned.
   ks_eps_solve with GD (EPSSetUp_XD davidson.c:51-77) returns KS_ERR_SUP for: ncv given and < nev; mpd > ncv or mpd < 2; nev + bs > ncv; the true
   residual, the two-sided flag, an extraction other than Ritz or arbitrary selection set; minv + bs > mpd; initial size > mpd; and, stated deviations
   from the reference, a non-symmetric problem type and B-orthogonalisation switched off with a B matrix. Defaults: ncv = max(nev, min(n - bs,
   max(2 nev, nev + 15)) + bs) (n + nev + bs for n < 10, mpd + nev + bs with mpd given), mpd = min(n, ncv), max_it = max(100 ncv, 2 n), `which` = largest
   magnitude, minv = min(max(bs, 6), mpd / 2), plusk = 1, initial size 6 (minv and initial size 1 for n < 10). Balancing is ignored. Further stated
   deviations (block sizes 1..16, one of lock / restart / expand per iteration, the restart test) are listed at the top of ks_gd.hip. The result
   getters, ks_eps_compute_error, the deflation space, the initial space (all its vectors up to the initial size), track-all, the monitor and the user's
   convergence and stopping functions work as after a LOBPCG solve. */
int ks_eps_gd_set_blocksize(ks_eps eps, int bs);          /* EPSGDSetBlockSize gd.c; 0 = default 1; outside 0..16: KS_ERR_ARG_OUTOFRANGE */
int ks_eps_gd_get_blocksize(ks_eps eps, int *bs);         /* EPSGDGetBlockSize */
int ks_eps_gd_set_restart(ks_eps eps, int minv, int plusk);   /* EPSGDSetRestart gd.c; minv 0 or -1 and plusk -1: the default */
int ks_eps_gd_get_restart(ks_eps eps, int *minv, int *plusk); /* EPSGDGetRestart: what was set, else what the last set-up resolved (minv 0 before one) */
int ks_eps_gd_set_initial_size(ks_eps eps, int initialsize);  /* EPSGDSetInitialSize gd.c; 0 or -1 = default */
int ks_eps_gd_get_initial_size(ks_eps eps, int *initialsize); /* EPSGDGetInitialSize */
int ks_eps_gd_set_borth(ks_eps eps, int borth);           /* EPSGDSetBOrth gd.c, default on; off with a B matrix: KS_ERR_SUP at the solve */
int ks_eps_gd_get_borth(ks_eps eps, int *borth);          /* EPSGDGetBOrth */
/* instrumentation of the last GD solve: passes of the main loop, restarts, locking steps, columns a matrix was applied to (A and B), columns
   preconditioned, calls of the fused Ritz-residual sweep */
int ks_eps_gd_get_stats(ks_eps eps, long long *iterations, long long *restarts, long long *locks, long long *mat_columns, long long *pc_columns, long long *fused_residuals);
/* KS_EPS_JD: Jacobi-Davidson (src/eps/impls/davidson/jd/jd.c and dvdimprovex.c; ks_jd.hip). The outer loop, the scope, the set-up rules with their
   KS_ERR_SUP cases and the choice of ST are GD's (above); the expansion vector of a pair (theta_j, u_j) is the approximate solution t of
       P K^-1 (theta1 A - theta0 B) t = -P K^-1 r_j,    P = I - Y (Zq^T Y)^-1 Zq^T,  Zq = B [X_locked, U],  Y = K^-1 Zq
   (dvd_improvex_jd_gen, dvdimprovex.c:590-700) with K the ST's preconditioner and (theta0, theta1) = (theta_j, 1) once ||r_j|| < fix |theta_j|, the
   target pair before (dvd_improvex_jd_lit_const_0). The inner solver is the ST's KSP type on this operator; where the caller has not chosen
   (ks_st_set_ksp_type, ks_st_set_ksp): BiCGStab, rtol 1e-4, at most 90 iterations (EPSSetDefaultST_JD, jd.c, which picks BiCGStab(l)). Reaching the limit
   or breaking down is no error: the iterate is the correction. The deviations from the reference are listed at the top of ks_jd.hip. JD keeps its own
   copy of the settings GD has. */
int ks_eps_jd_set_blocksize(ks_eps eps, int bs);          /* EPSJDSetBlockSize jd.c; as ks_eps_gd_set_blocksize */
int ks_eps_jd_get_blocksize(ks_eps eps, int *bs);         /* EPSJDGetBlockSize jd.c */
int ks_eps_jd_set_restart(ks_eps eps, int minv, int plusk);   /* EPSJDSetRestart jd.c */
int ks_eps_jd_get_restart(ks_eps eps, int *minv, int *plusk); /* EPSJDGetRestart jd.c */
int ks_eps_jd_set_initial_size(ks_eps eps, int initialsize);  /* EPSJDSetInitialSize jd.c */
int ks_eps_jd_get_initial_size(ks_eps eps, int *initialsize); /* EPSJDGetInitialSize jd.c */
int ks_eps_jd_set_borth(ks_eps eps, int borth);           /* EPSJDSetBOrth jd.c */
int ks_eps_jd_get_borth(ks_eps eps, int *borth);          /* EPSJDGetBOrth jd.c */
int ks_eps_jd_set_fix(ks_eps eps, double fix);            /* EPSJDSetFix jd.c: default 0.01; fix <= 0: KS_ERR_ARG_OUTOFRANGE */
int ks_eps_jd_get_fix(ks_eps eps, double *fix);           /* EPSJDGetFix jd.c */
int ks_eps_jd_set_const_correction_tol(ks_eps eps, int constant);   /* EPSJDSetConstCorrectionTol jd.c: default on; off: the dynamic tolerance of dvdimprovex.c:603-605 (0.5, halved after each outer iteration that solved a correction, floor 10 eps, 0.5 again after a lock) */
int ks_eps_jd_get_const_correction_tol(ks_eps eps, int *constant);  /* EPSJDGetConstCorrectionTol jd.c */
/* instrumentation of the last JD solve: the first five as ks_eps_gd_get_stats (the products and preconditioner applications of the inner solves
   included), then the correction equations solved (dvd_improvex_jd_gen), their Krylov iterations, and the pairs that took the GD correction instead
   (dvdimprovex.c:650-655, 683-690) */
int ks_eps_jd_get_stats(ks_eps eps, long long *iterations, long long *restarts, long long *locks, long long *mat_columns, long long *pc_columns,
                        long long *inner_solves, long long *inner_iterations, long long *gd_fallbacks);
int ks_eps_set_track_all(ks_eps eps, int trackall);                          /* EPSSetTrackAll: error estimates of all Ritz pairs at every restart (for monitors) */
int ks_eps_get_krylovschur(ks_eps eps, double *keep, int *lock);             /* EPSKrylovSchurGetRestart / EPSKrylovSchurGetLocking */
int ks_eps_set_balance(ks_eps eps, int bal, int its, double cutoff);        /* EPSSetBalance epsopts.c:1050 (non-symmetric problems; EPSBuildBalance_Krylov epsdefault.c:370); its / cutoff 0 keep 5 / 1e-8 */
int ks_eps_set_balance_matrix(ks_eps eps, const double *D_dev);             /* STSetBalanceMatrix on the solver's ST: EPS_BALANCE_USER with this diagonal (device, n_local, copied) */
int ks_eps_get_balance(ks_eps eps, int *bal, int *its, double *cutoff);
int ks_eps_set_true_residual(ks_eps eps, int trueres);                    /* EPSSetTrueResidual: convergence on ||A x - k B x|| of the Ritz vector (epskrylov.c:256-264) */
int ks_eps_get_true_residual(ks_eps eps, int *trueres);
int ks_eps_get_operators(ks_eps eps, ks_mat *A, ks_mat *B);
int ks_eps_get_problem_type(ks_eps eps, int *type, int *generalized, int *hermitian, int *positive);
int ks_eps_get_bv(ks_eps eps, ks_bv *V);
/* arnoldi_steps and gs_passes of a two-sided solve count the steps and passes of both runs (Op on the right basis, Op^T on the left) */
int ks_eps_get_stats(ks_eps eps, long long *arnoldi_steps, long long *gs_passes, int *restarts);
/* EPSSetTwoSided (epsopts.c) with EPSGetLeftEigenvector (epssolve.c:567): two-sided Krylov-Schur (ks-twosided.c; Zwaan and Hochstenbach 2017) for
   non-symmetric problems. Every restart runs two Arnoldi expansions through ks_bv_matarnoldi, one with Op and one with Op^T (ks_mat_create_transpose
   of the solver's operator: A must have a transposed product, KS_MAT_KEEP_CSR or a shell with ks_mat_shell_set_mult_transpose; checked at set-up),
   and solves the two projected problems together (DS NHEPTS). Convergence is the larger of the right and the left estimate, ks_eps_compute_error
   the larger of the right residual and the left one, ||A^T y - conj(k) B^T y|| (epssolve.c:692-711). Left eigenvectors satisfy y^H A = k y^H B: for
   a conjugate pair (yr, yi) of the first member and (yr, -yi) of the second, each normalised to unit 2-norm as a complex vector. With a B matrix
   (KS_EPS_GNHEP; the inner product stays the standard one) the converged left vectors go through P^-T before they are normalised
   (EPSComputeVectors_Twosided epsdefault.c:79-95, ks_st_matsolve_transpose).
   ks_eps_solve returns KS_ERR_SUP with the flag set when
     - the problem type is KS_EPS_HEP or KS_EPS_GHEP (the reference's own check, epssetup.c:309)
     - a B matrix is set and the EPS's ST has no transposed solves (ks_st_set_transpose_solves)
     - the ST is not STSHIFT and has no transposed solves (sinvert and Cayley need solves with the transposed matrix)
     - balancing is on
     - the extraction is harmonic
     - the true residual is asked for
     - a deflation space is set
     - the context has more than one rank and the operator has no transposed product across ranks: that takes a matrix created with
       KS_MAT_SHARDED_TRANSPOSE, STSHIFT (any shift) and no B matrix; transposed ST solves are one rank, so sinvert, Cayley and B stay refused
       there. Every rank refuses at the same point, before any collective. Left eigenvectors are returned as each rank's local part.
   Without the flag ks_eps_get_left_eigenvector returns the right eigenvector for KS_EPS_HEP / KS_EPS_GHEP (the left one of a symmetric problem)
   and KS_ERR_ARG_WRONGSTATE for a non-symmetric one. */
int ks_eps_set_two_sided(ks_eps eps, int twosided);
int ks_eps_get_two_sided(ks_eps eps, int *twosided);
int ks_eps_set_left_initial_space(ks_eps eps, int n, const double *const *w_dev);   /* EPSSetLeftInitialSpace: device vectors; the first starts the left recurrence */
int ks_eps_get_left_eigenvector(ks_eps eps, int i, double *yr_dev, double *yi_dev);  /* device vectors of n_local doubles; either may be NULL */
int ks_eps_get_left_eigenvector_host(ks_eps eps, int i, double *yr_host, double *yi_host);
/* instrumentation: restarts of the last two-sided solve whose two projected halves came out of the sort in different orders (eigenvalues that tie
   under the criterion) and had the second half permuted to match the first (DSSort_NHEPTS dsnhepts.c:216-231) */
int ks_eps_get_two_sided_stats(ks_eps eps, long long *ds_permutations);

/* ---- ST: spectral transformation (slepcst.h) ---------------------------------------------------
   STSHIFT and STSINVERT in matrix mode "shell" (A - sigma*B is applied, never assembled); the linear solves are
   GMRES(restart) + Jacobi, the KSP that mode defaults to (stsles.c:51-53), run on the BV kernels of this library.
   An EPS owns one ST (ks_eps_get_st = EPSGetST); ks_st_create makes a stand-alone one. */
int ks_st_create(ks_ctx ctx, ks_st *st);
int ks_st_destroy(ks_st st);
int ks_st_set_type(ks_st st, int type);                                   /* STSetType */
int ks_st_set_shift(ks_st st, double sigma);                              /* STSetShift */
int ks_st_get_shift(ks_st st, double *sigma);
int ks_st_cayley_set_antishift(ks_st st, double nu);                      /* STCayleySetAntishift cayley.c:236 (default: the shift) */
int ks_st_cayley_get_antishift(ks_st st, double *nu);
int ks_st_set_matrices(ks_st st, ks_mat A, ks_mat B /* may be NULL */);   /* STSetMatrices */
/* STSetMatMode (src/sys/classes/st/interface/stfunc.c): how the matrix of the linear solves, P = A - sigma B, exists.
   KS_ST_MATMODE_SHELL (the default here, with the KSP that mode defaults to, stsles.c:51-53): never assembled, applied as two products and
   an axpy (stshellmat.c). KS_ST_MATMODE_COPY (the reference's default mode): assembled once per shift by ks_mat_create_axpy (STMatMAXPY_Private
   stsolve.c:603-631) - one product per application, the Jacobi diagonal is MatGetDiagonal of it; A and B need KS_MAT_KEEP_CSR. The solver
   around it is the same (GMRES / BiCGStab + Jacobi). ST_MATMODE_INPLACE (A overwritten) is not built. The M of cayley / shift stays in the
   term-by-term form in either mode. */
#define KS_ST_MATMODE_COPY  0
#define KS_ST_MATMODE_SHELL 2
int ks_st_set_matmode(ks_st st, int mode);
int ks_st_get_matmode(ks_st st, int *mode);
/* KS_KSP_PREONLY is KSPPREONLY: the solve is ONE application of the preconditioner - no residual, no convergence test, no Krylov basis - which is
   exact with KS_PC_LU (the reference's default pair, -st_ksp_type preonly -st_pc_type lu) and allowed with every PC type, as in PETSc.
   ks_st_get_ksp_stats counts one solve and one iteration per application and leaves last_rnorm alone. */
/* KS_KSP_CG is KSPCG (-st_ksp_type cg, ex11.c's second test) with the preconditioner on the left and PETSc's default norm for it, the preconditioned
   residual: y = 0, r = b, z = M^-1 r, tol = max(rtol ||z||, 1e-50); per iteration gamma = (r,z), p = z + (gamma / gamma_old) p, w = P p,
   delta = (p,w), alpha = gamma / delta, y += alpha p, r -= alpha w, z = M^-1 r, converged when ||z|| <= tol. For a symmetric positive definite P
   and M: the symmetry is the caller's business, as in PETSc. One product and 12 vector passes per iteration, four work vectors. The KSP of the ST
   is strict: KS_ERR_NOT_CONVERGED when (p,w) <= 0 ("indefinite matrix"), (r,z) < 0 ("indefinite preconditioner"), either is not finite ("not a
   number") or max_it is reached ("reached %d iterations"). Every transformation with a solve, both matrix modes, every PC type, the transposed
   side (ks_st_set_transpose_solves) and, with the PC types that have it, more than one rank. A Jacobi-Davidson solve whose ST has it set is
   KS_ERR_SUP at set-up (its projected operator is not symmetric as applied). A zero right-hand side gives y = 0 and counts no iteration.
   Its value is 4: the value 3 names no solver and stays KS_ERR_SUP, which is what callers of earlier versions got for it. */
/* KS_KSP_MINRES is KSPMINRES (-st_ksp_type minres) after Paige and Saunders, for a symmetric P that may be indefinite - shift-and-invert at a target
   inside the spectrum - with a symmetric positive definite preconditioner M applied symmetrically. The norm it minimises, tests and reports as
   last_rnorm is phibar = ||b - P y|| in the M^-1 inner product:
     y = 0; r1 = r2 = b; z = M^-1 b; beta1 = sqrt((b,z)); tol = max(rtol beta1, 1e-50); beta = beta1; phibar = beta1; cs = -1; sn = dbar = epsln = 0
     iteration i:  v = z / beta;  u = P v;  if i > 0: u -= (beta / oldb) r1;  alfa = (v,u);  u -= (alfa / beta) r2;  r1 = r2; r2 = u;  z = M^-1 r2
                   oldb = beta;  beta = sqrt((r2,z));  oldeps = epsln;  delta = cs dbar + sn alfa;  gbar = sn dbar - cs alfa;  epsln = sn beta
                   dbar = -cs beta;  gamma = max(hypot(gbar, beta), DBL_EPSILON);  cs = gbar / gamma;  sn = beta / gamma;  phi = cs phibar
                   phibar = sn phibar;  w1 = w2; w2 = w;  w = (v - oldeps w1 - delta w2) / gamma;  y += phi w;  converged when phibar <= tol
   One product and 16 vector passes per iteration, seven work vectors, no restart. The KSP of the ST is strict: KS_ERR_NOT_CONVERGED when (b,z) or
   (r2,z) < 0 ("indefinite preconditioner": point Jacobi of an indefinite P has negative entries, see ks_st_pc_jacobi_set_use_abs), alfa or either
   inner product is not finite ("not a number") or max_it is reached ("reached %d iterations"). beta = 0 after an iteration is the lucky breakdown:
   phibar = 0, converged. Supported where KS_KSP_CG is: every transformation with a solve, both matrix modes, every PC type, the transposed side
   and, with the PC types that have it, more than one rank; a Jacobi-Davidson solve whose ST has it set is KS_ERR_SUP at set-up. A zero right-hand
   side gives y = 0 and counts no iteration. The symmetry of P and M is the caller's business.
   Its value is 6: the values 3 and 5 name no solver and stay KS_ERR_SUP, which is what callers of earlier versions got for them. */
/* KS_KSP_BCGSL is KSPBCGSL (-st_ksp_type bcgsl), the BiCGStab(l) of Sleijpen and Fokkema, for a P that need not be symmetric: l BiCG steps, then one
   minimum-residual polynomial of degree l, whose roots may be complex pairs - where BiCGStab's one-step polynomial with its real root stagnates or
   breaks down (convection-dominated operators, A - sigma I with the target inside a non-symmetric spectrum). 2 l + 4 work vectors, no restart. The
   preconditioner is on the left, A^ = M^-1 P, and the norm that is tested and reported as last_rnorm is the preconditioned residual, as for KS_KSP_BCGS:
     y = 0; r_0 = M^-1 b; rt = r_0; u_0 = 0; rho0 = 1; alpha = 0; omega = 1; dp0 = ||r_0||; tol = max(rtol dp0, 1e-50)
     cycle:  converged when ||r_0|| <= tol; its >= max_it: "reached %d iterations"                 (both tested at the start of a cycle only)
             rho0 = -omega rho0
             for j = 0 .. l-1:  rho1 = (r_j, rt); beta = alpha (rho1 / rho0); rho0 = rho1;  u_i = r_i - beta u_i (i <= j);  u_{j+1} = A^ u_j
                                sigma = (u_{j+1}, rt); alpha = rho1 / sigma;  y += alpha u_0;  r_i -= alpha u_{i+1} (i <= j);  r_{j+1} = A^ r_j
             G = [r_0 .. r_l]^T [r_0 .. r_l];  gamma = argmin ||r_0 - sum_j gamma_j r_j||  (Cholesky of G(1:l,1:l), right-hand side G(1:l,0))
             y += sum gamma_j r_{j-1};  r_0 -= sum gamma_j r_j;  u_0 -= sum gamma_j u_j;  omega = gamma_l
   ks_st_get_ksp_stats counts BiCG steps as iterations, l per cycle (two products each); last_rnorm is ||M^-1 (b - P y)|| as the recurrence has it after
   the last minimum-residual step. The KSP of the ST is strict: KS_ERR_NOT_CONVERGED when rho0 or sigma is zero ("breakdown"), a Cholesky pivot is
   <= 0 ("singular minimum-residual step"), a value is not finite ("not a number") or max_it is reached ("reached %d iterations"). Not built:
   PETSc's convex polynomial (KSPBCGSLSetPol), its residual replacement (KSPBCGSLSetXRes) and the pseudo-inverse (KSPBCGSLSetUsePseudoinverse).
   Supported where KS_KSP_CG is: every transformation with a solve, both matrix modes, every PC type, the transposed side and, with the PC types
   that have it, more than one rank; a Jacobi-Davidson solve whose ST has it set is KS_ERR_SUP at set-up (the device-resident solvers run on the
   ST's own operator, not on the projected one). A zero right-hand side gives y = 0 and counts no iteration.
   Its value is 8: the values 3, 5 and 7 name no solver and stay KS_ERR_SUP. */
enum { KS_KSP_GMRES = 0, KS_KSP_BCGS = 1, KS_KSP_PREONLY = 2, KS_KSP_CG = 4, KS_KSP_MINRES = 6, KS_KSP_BCGSL = 8 };
int ks_st_set_ksp_type(ks_st st, int type);                                /* KSPSetType on STGetKSP: GMRES (restarted, the shell mode's default), BiCGStab, BiCGStab(l), CG - all preconditioned on the left -, MINRES or PREONLY; any other value: KS_ERR_SUP */
/* KS_KSP_BCGSL: l of BiCGStab(l) (KSPBCGSLSetEll), 1..4 (KS_ERR_ARG_OUTOFRANGE otherwise), default 2; l = 1 is a device-resident BiCGStab. The setter
   clears the set-up: the work vectors depend on l. */
int ks_st_bcgsl_set_ell(ks_st st, int ell);
int ks_st_bcgsl_get_ell(ks_st st, int *ell);
/* KS_KSP_BCGSL has the device-resident form of KS_KSP_CG (below) with a check interval and counters of its own. The interval counts CYCLES of l steps:
   1..1024 (KS_ERR_ARG_OUTOFRANGE otherwise), default 4; count, solution and last_rnorm are the same bits for every c. gated_iterations counts cycles. */
int ks_st_bcgsl_set_check_interval(ks_st st, int c);
int ks_st_bcgsl_get_check_interval(ks_st st, int *c);
int ks_st_bcgsl_get_stats(ks_st st, long long *sweeps, long long *host_waits, long long *gated_cycles);
/* KS_KSP_MINRES has the device-resident form of KS_KSP_CG (below) with a check interval and counters of its own: setting one solver's leaves the other's alone. */
int ks_st_minres_set_check_interval(ks_st st, int c);                      /* 1..1024 (KS_ERR_ARG_OUTOFRANGE otherwise), default 8; count, solution and last_rnorm are the same bits for every c */
int ks_st_minres_get_check_interval(ks_st st, int *c);
int ks_st_minres_get_stats(ks_st st, long long *sweeps, long long *host_waits, long long *gated_iterations);
/* PCJacobiSetUseAbs (-pc_jacobi_abs): with flag != 0 KS_PC_JACOBI scales by 1 / |diag(P)|, a positive definite M whatever the signs of the diagonal -
   what MINRES needs on an indefinite P. A zero entry still leaves its row unscaled. Default off, and off gives the diagonal of earlier versions bit
   for bit. The setter clears the set-up. No effect on the other PC types. */
int ks_st_pc_jacobi_set_use_abs(ks_st st, int flag);
int ks_st_pc_jacobi_get_use_abs(ks_st st, int *flag);
/* KS_KSP_CG keeps its scalars on the device and switches itself off there once a solve has ended: the host enqueues c iterations, then reads the
   solver's state once. c: 1..1024 (KS_ERR_ARG_OUTOFRANGE otherwise), default 8; c = 1 is the classic loop with one host test per iteration. The
   iteration count, the solution and last_rnorm are the same bits for every c. */
int ks_st_cg_set_check_interval(ks_st st, int c);
int ks_st_cg_get_check_interval(ks_st st, int *c);
/* Since the ST was created (any pointer may be NULL): launches of the solver's own kernels, host reads of the device state, and iterations that were
   enqueued but switched themselves off on the device because the solve had already ended. */
int ks_st_cg_get_stats(ks_st st, long long *sweeps, long long *host_waits, long long *gated_iterations);
/* KSPGMRESSetCGSRefinementType on STGetKSP, with the BV constants: KS_BV_ORTHOG_REFINE_NEVER (PETSc's default for KSPGMRES: one pass of
   classical Gram-Schmidt, then the norm), _IFNEEDED (PETSc's test is the BV's, eta 0.7071) or _ALWAYS */
int ks_st_set_gmres_cgs_refinement(ks_st st, int refine);
/* PCSetType on KSPGetPC(STGetKSP): KS_PC_NONE (no preconditioner), KS_PC_JACOBI (the default: PCJACOBI, what the shell matrix mode defaults to, stsles.c:51-53) or
   KS_PC_BJACOBI - PCBJACOBI (the reference's choice with a split preconditioner, stsles.c:46-48; -st_pc_type bjacobi in ex46.c:113,
   test34.c:113) with blocks of block_size consecutive local rows (-pc_bjacobi_local_blocks n_local/block_size) solved exactly
   (-sub_pc_type lu): the dense diagonal blocks of P = A - sigma B are inverted on the host at STSetUp and applied by one kernel.
   2 <= block_size <= 32; the matrices must hold their CSR arrays (KS_MAT_KEEP_CSR); a singular block is KS_ERR_MAT_LU_ZRPVT.
   KS_PC_BJACOBI_ILU - PCBJACOBI with -sub_pc_type ilu at zero fill, PETSc's parallel default for AIJ matrices (PCSetUp_BJacobi; the sub-solver is
   MatILUFactor with levels 0 in natural ordering): blocks of block_size consecutive local rows, the last one of a rank as short as one row,
   columns outside the block dropped; each block is factored on its own pattern on the host at STSetUp (IKJ order, no pivoting, no fill) and
   applied by two level-scheduled sparse triangular solves, one workgroup per block with the block's vector in LDS.
   64 <= block_size <= 8192 (KS_ERR_ARG_OUTOFRANGE otherwise); the matrices must hold their CSR arrays (KS_ERR_ORDER at set-up); a row of a block
   without a stored diagonal entry is KS_ERR_ARG_WRONGSTATE ("Matrix is missing diagonal entry"), a zero pivot KS_ERR_MAT_LU_ZRPVT. */
#define KS_PC_JACOBI  0
#define KS_PC_BJACOBI 1
#define KS_PC_BJACOBI_ILU 2
#define KS_PC_NONE 3         /* -st_pc_type none: M = I; takes block_size 0 (anything else is KS_ERR_SUP: there is no blocked form of it) */
/* KS_PC_LU - PCLU (PETSc's built-in sequential sparse LU, the reference's default inner solver with KSPPREONLY: stsles.c, -st_pc_type lu): the whole
   P = A - sigma B (or B, for a shift with two matrices) is factored WITH fill on the host, Q P Q^T = L U, under a nested dissection ordering Q
   applied symmetrically and without pivoting (-pc_factor_mat_ordering_type nd, PCLU's default); the application y = Q^T U^-1 L^-1 Q x runs on
   the device level by level. Takes block_size 0 (anything else is KS_ERR_SUP, as for KS_PC_NONE). At set-up: the matrices must hold their CSR
   arrays (KS_MAT_KEEP_CSR; KS_ERR_ORDER); more than one rank is KS_ERR_SUP (PETSc's built-in LU is sequential as well); a zero pivot is
   KS_ERR_MAT_LU_ZRPVT with the original row in the message; factors with more than 2^31 - 1 stored entries, or a failed host or device
   allocation, are KS_ERR_MEM with nothing left half-built. With ks_st_set_transpose_solves a second plan of the same factors serves
   y = Q^T L^-T U^-T Q x. The default preconditioner stays point Jacobi. */
#define KS_PC_LU 4
/* KS_PC_AMG - smoothed-aggregation algebraic multigrid (PCGAMG with -pc_gamg_type agg, -st_pc_type gamg; written from the algorithm's description): a
   hierarchy of P = A - sigma B (or B) made on the host - a symmetrised strength graph with threshold theta, aggregates in three ascending passes,
   the prolongator (I - 4/(3 rho) D^-1 A) T of the piecewise constant T, R = P^T, Galerkin operators R A P, the last level (at most coarse_limit
   rows, or the max_levels-th, or one that no longer coarsens) factored like KS_PC_LU - and on the device one V(nu, nu) cycle per application with
   nu Chebyshev steps on D^-1 A over [0.1 rho, rho], rho being Gershgorin's bound. The cycle is symmetric for a symmetric P. Takes block_size 0
   (anything else is KS_ERR_SUP). At set-up: the matrices must hold their CSR arrays (KS_MAT_KEEP_CSR; KS_ERR_ORDER); more than one rank, or
   ks_st_set_transpose_solves, is KS_ERR_SUP (ks_st_pc_apply_transpose too); a row of any level without a stored diagonal entry, or with a zero
   one, is KS_ERR_ARG_WRONGSTATE with the row in the message; a zero pivot of the last level KS_ERR_MAT_LU_ZRPVT; a product with more than
   2^31 - 1 entries KS_ERR_ARG_OUTOFRANGE, a failed allocation KS_ERR_MEM, with nothing left half-built. The default stays point Jacobi. */
#define KS_PC_AMG 5
int ks_st_set_pc(ks_st st, int type, int block_size);
/* The options of KS_PC_AMG; every setter clears the set-up, a value out of range is KS_ERR_ARG_OUTOFRANGE.
   threshold: theta of the strength test |a_ij| >= theta sqrt(|a_ii a_jj|), 0 <= theta < 1, default 0 (-pc_gamg_threshold).
   smoother: Chebyshev steps nu before and after the coarse correction, 1..4, default 2 (-mg_levels_ksp_max_it).
   coarse: a level with at most coarse_limit (>= 1, default 200) rows is solved directly (-pc_gamg_coarse_eq_limit); at most max_levels levels,
   1..16, default 10 (-pc_mg_levels).
   prolongator smoothing: on by default (-pc_gamg_agg_nsmooths 1); off: the plain aggregation prolongator T. */
int ks_st_pc_amg_set_threshold(ks_st st, double theta);
int ks_st_pc_amg_get_threshold(ks_st st, double *theta);
int ks_st_pc_amg_set_smoother(ks_st st, int degree);
int ks_st_pc_amg_get_smoother(ks_st st, int *degree);
int ks_st_pc_amg_set_coarse(ks_st st, int coarse_limit, int max_levels);
int ks_st_pc_amg_get_coarse(ks_st st, int *coarse_limit, int *max_levels);
int ks_st_pc_amg_set_prolongator_smoothing(ks_st st, int on);
int ks_st_pc_amg_get_prolongator_smoothing(ks_st st, int *on);
/* The hierarchy. Any pointer may be NULL. levels; rows, nnz, rho: per level, arrays of 16 (rho of the last level is 0: it is not smoothed);
   complexity: stored entries of all the operators over those of the first; device_bytes: everything the preconditioner holds on the device;
   launches: per application of one vector, a matrix product counted as one. Runs the set-up if needed; KS_ERR_ORDER when the PC is not KS_PC_AMG
   or the transformation has no solve. */
int ks_st_pc_amg_get_info(ks_st st, int *levels, int *rows, long long *nnz, double *rho, double *complexity, long long *device_bytes, int *launches);
/* One level on the host, in two steps: with the arrays NULL only n, n_coarse (0 on the last level) and the stored entries of the level's operator
   and of its prolongator are returned; then arp (n + 1), acol, aval (nnz_a), prp (n + 1), pcol, pval (nnz_p) and agg (n: the aggregate of a row, -1
   outside every aggregate) are filled - the A group, the P group and agg each only when given; on the last level prp is all 0 and agg all -1. */
int ks_st_pc_amg_get_level(ks_st st, int level, int *n, int *n_coarse, long long *nnz_a, long long *nnz_p, int *arp, int *acol, double *aval,
                           int *prp, int *pcol, double *pval, int *agg);
/* Test hook (KSD_TEST_HOOKS): one transfer kernel of KS_PC_AMG on a rectangular CSR matrix M given in host arrays (nrows x ncols, nvec vectors,
   column-major). restriction != 0: out = M (u - v), u and v ncols x nvec; else out = v + M u, u ncols x nvec, v nrows x nvec. lanes: lanes per
   row, 1, 8 or 64, 0 = the library's choice. All arrays in host memory. */
int ks_pc_amg_test_transfer(ks_ctx ctx, int restriction, int lanes, int nrows, int ncols, const int *rp, const int *col, const double *val,
                            int nvec, const double *u_host, const double *v_host, double *out_host);
/* -pc_factor_mat_ordering_type on the PCLU: KS_ORDERING_ND (the default, as PCLU's: George's automatic nested dissection on rooted level structures
   of the graph of P + P^T, MATORDERINGND) or KS_ORDERING_NATURAL; any other value is KS_ERR_ARG_OUTOFRANGE. Changing it clears the set-up. */
#define KS_ORDERING_ND      0
#define KS_ORDERING_NATURAL 1
int ks_st_pc_lu_set_ordering(ks_st st, int which);
int ks_st_pc_lu_get_ordering_type(ks_st st, int *which);
/* The row permutation of the factorisation (MatGetOrdering / ISGetIndices on the PCLU's ordering): perm_host[i] (n ints, host memory) is the original
   row eliminated i-th. Runs the set-up if needed; KS_ERR_ORDER when the PC is not KS_PC_LU or the transformation has no solve. */
int ks_st_pc_lu_get_permutation(ks_st st, int *perm_host);
/* MatGetInfo on the factor (nz_used, PCFactor's fill) plus this library's schedule. Any pointer may be NULL. n; nnz_l: stored entries of L without its
   unit diagonal; nnz_u: of U with the diagonal; levels_l, levels_u: levels of the two triangular solves; wide: the threshold in rows from which a
   level is a launch of its own; wide_launches, narrow_launches: launches of the two kinds per forward application (both triangles); device_bytes:
   everything the preconditioner holds on the device (the transposed plan included). Runs the set-up if needed; errors as above. */
int ks_st_pc_lu_get_info(ks_st st, int *n, long long *nnz_l, long long *nnz_u, int *levels_l, int *levels_u, int *wide, int *wide_launches, int *narrow_launches,
                         long long *device_bytes);
/* MatGetInertia on the factor: the numbers of negative and positive pivots u_rr; *zero is always 0, a zero pivot having failed the set-up. This is the
   inertia of P = A - sigma B ONLY WHEN P IS SYMMETRIC (Sylvester's law applied to L D L^T = L U); for a non-symmetric P the counts are just the signs of
   the pivots. Runs the set-up if needed; errors as above. */
int ks_st_pc_lu_get_inertia(ks_st st, int *neg, int *zero, int *pos);
int ks_st_set_ksp(ks_st st, double rtol, int max_it, int restart);        /* KSPSetTolerances / KSPGMRESSetRestart on STGetKSP; 0 keeps */
int ks_st_setup(ks_st st);                                                /* STSetUp */
int ks_st_apply(ks_st st, const double *x_dev, double *y_dev);            /* STApply stsolve.c:44 */
/* STApplyTranspose / STApplyHermitianTranspose (stsolve.c:107-116, :153-162; real scalars). Shift with one matrix: y = (A - sigma I)^T x
   (MatMultTranspose of A), always. The transformations with a solve need it with the transposed matrix: KS_ERR_SUP unless the ST has transposed
   solves (ks_st_set_transpose_solves), then by STApplyTranspose_Generic
       sinvert, 1 matrix    y = P^-T x                  sinvert, 2 matrices  w = P^-T x, y = B^T w
       cayley               w = P^-T x, y = (A + nu B)^T w   (B = I with one matrix)
       shift, 2 matrices    w = B^-T x, y = (A - sigma B)^T w */
int ks_st_apply_transpose(ks_st st, const double *x_dev, double *y_dev);
/* Solves with the transposed matrix (STMatSolveTranspose stsolve.c, on PETSc's KSPSolveTranspose and PCApplyTranspose), prepared ON REQUEST:
   enable = 0 is the default, and with it every code path, error code and device allocation of the ST is what it was before this switch existed.
   With enable != 0 STSetUp also prepares the transposed side: the transposed matrices of A and B (ks_mat_create_transpose; shell mode) or of the
   assembled P, which then keeps its CSR arrays (copy mode), and for KS_PC_BJACOBI_ILU a second level plan of the same factors - the device bytes
   of the factors double. That cost is why this is a switch; the default may flip in a later change. Set-up errors with the switch on: KS_ERR_ORDER
   when A or B did not keep its CSR arrays (KS_MAT_KEEP_CSR), KS_ERR_SUP on more than one rank (the transpose of a row-sharded matrix is a
   redistribution). Changing the switch clears the set-up. With it on, ks_st_apply_transpose works for every transformation, two-sided
   Krylov-Schur accepts sinvert, Cayley and a B matrix, and two-sided balancing works behind a solve. */
int ks_st_set_transpose_solves(ks_st st, int enable);
int ks_st_get_transpose_solves(ks_st st, int *enable);
/* STMatSolveTranspose (stsolve.c): P^T y = b with the KSP of the ST on its transposed side (KSPSolveTranspose: the same left-preconditioned
   iteration on M^-T P^T y = M^-T b, PCApplyBAorABTranspose with PC_LEFT); P = A - sigma B for sinvert and Cayley, P = B for a shift with two
   matrices. ks_st_get_ksp_stats counts these solves with the others. KS_ERR_SUP without ks_st_set_transpose_solves; KS_ERR_ORDER for STSHIFT with
   one matrix (no linear solve); b == y is KS_ERR_ARG_IDN. */
int ks_st_matsolve_transpose(ks_st st, const double *b_dev, double *y_dev);
/* PCApplyTranspose on KSPGetPC(STGetKSP) (PETSc's, as PCApply): y = M^-T x. Point Jacobi is its own transpose; the dense blocks are applied by
   columns of the same inverses; the ILU(0) blocks use the SAME factors, y = L^-T U^-T x (not an ILU(0) of P^T), from their transposed level plan.
   Same errors as ks_st_matsolve_transpose. Enqueued on the context's stream, no host wait. */
int ks_st_pc_apply_transpose(ks_st st, const double *x_dev, double *y_dev);
/* PCApply on KSPGetPC(STGetKSP) (the KSP of stsles.c:51-58; PCApply itself is PETSc's, external to the reference): y = M^-1 x with the
   preconditioner of the inner solves, whichever type is set. Runs STSetUp if needed; x == y is KS_ERR_ARG_IDN; a transformation
   without a linear solve (STSHIFT with one matrix) has no preconditioner: KS_ERR_ORDER. Enqueued on the context's stream, no host wait. */
int ks_st_pc_apply(ks_st st, const double *x_dev, double *y_dev);
/* KS_ST_PRECOND (STPRECOND, src/sys/classes/st/impls/precond/precond.c): the ST of the preconditioned eigensolvers. ks_st_apply gives y = M^-1 x with the
   preconditioner M built on K = A - sigma B, sigma the shift, or the EPS's target when none was set (precond.c:65); the KSP is preonly, nothing is
   solved. Default PC: point Jacobi (what the shell matrix mode defaults to, precond.c:30); every PC type works, KS_PC_LU being the exact K^-1. ks_st_backtransform leaves values alone.
   PCMatApply on KSPGetPC(STGetKSP): Y(:,j) = M^-1 X(:,j), j < ncols (X(:,j) at X_dev + j*ldx, Y(:,j) at Y_dev + j*ldy), every column bit for bit
   ks_st_pc_apply of that column. Point Jacobi, PCNONE and the dense blocks run their single-vector kernels with the column on the grid; the ILU(0)
   blocks of up to 512 rows keep eight right-hand sides of a block in LDS at once, read every factor entry once for all of them and pay one barrier
   per level instead of one per level and column (more columns go in several passes); larger blocks go column by column through the single-vector
   kernel, which measured no slower there (ks_pc.hip).
   Arguments as ks_mat_mult_multi: ncols == 0 does nothing, ldx, ldy >= max(1, n_local) (KS_ERR_ARG_SIZ), X and Y must not overlap
   (KS_ERR_ARG_WRONG). Enqueued, no host wait. */
int ks_st_pc_apply_multi(ks_st st, int ncols, const double *X_dev, int ldx, double *Y_dev, int ldy);
int ks_st_pc_multi_columns(ks_st st, int *columns);   /* instrumentation: columns of one pass of the above with the PC as set up (ILU blocks: 8 up to block size 512, 1 above; KS_PC_LU: 8 - a narrow stage of the schedule keeps eight right-hand sides in one launch, a wide level puts them on the grid; KS_PC_AMG: 8 - the level operators' block product and the work vectors of the cycle; the other types: 65535, one launch) */
/* STApplyMat stsolve.c:62: Y(:,j) = Op X(:,j). KS_ST_PRECOND: ks_st_pc_apply_multi; the other transformations: ks_st_apply column by column. Same arguments. */
int ks_st_apply_mat(ks_st st, int ncols, const double *X_dev, int ldx, double *Y_dev, int ldy);
int ks_st_backtransform(ks_st st, int n, double *eigr, double *eigi);     /* STBackTransform stsolve.c:563 */
int ks_st_get_ksp_stats(ks_st st, long long *solves, long long *iterations, double *last_rnorm);   /* solves and iterations of every KSP type since the ST was created; last_rnorm: the preconditioned residual norm of the last solve (KS_KSP_MINRES: its phibar) */

/* ---- profiling: HIP-event timing per kernel class, on the context's stream -------------------- */
/* A class is one __global__ kernel template; `variant` is its compile-time column tile KT (0 when
   the kernel has none), so (class, variant) names ONE kernel symbol as rocprofv3 reports it.
   Launches of the speculative Gram-Schmidt slots that gated themselves off on the device are
   re-filed under KS_K_NOOP once the host has read back the pass counts.                          */
enum { KS_K_SPMV = 0, KS_K_DOT, KS_K_GSFIN, KS_K_UPD_FUSED, KS_K_UPD, KS_K_SCALE, KS_K_MULTINPLACE, KS_K_COPY,
       KS_K_MULT, KS_K_BVDOT, KS_K_NORM, KS_K_HALO, KS_K_ALLREDUCE, KS_K_NOOP, KS_K_OTHER,
       KS_K_SPMVDOT /* MatMult fused into the dot sweep that follows it (cache-resident bases, dictionary layout) */, KS_K_COUNT };
#define KS_PROF_VARIANTS 65      /* variant = KT in 0..64 (every count up to 32 is compiled, then 40, 48, 56, 64) */
int ks_prof_enable(ks_ctx ctx, int on);   /* 0: off, 1: every class, else a mask with bit (class+1) set per class to time */
int ks_prof_reset(ks_ctx ctx);
/* launches, summed elapsed ms, summed algorithmic bytes (SURVEY.md 8d formulas) and summed compulsory
   HBM bytes (what the kernel as designed must move) of one class; variant<0 sums over all variants */
int ks_prof_get(ks_ctx ctx, int kclass, int variant, long long *launches, double *ms, double *alg_bytes, double *hbm_bytes);
const char *ks_prof_class_name(int kclass);
/* the reference's log event under which -log_view shows that class's work (bvfunc.c:69-86: BVMatMultVec, BVDotVec, BVMultVec, BVScale, BVMultInPlace,
   BVOrthogonalizeV ...; a fused launch names both events it does the work of, e.g. "BVMultVec+BVDotVec") */
const char *ks_prof_event_name(int kclass);

#ifdef __cplusplus
}
#endif
#endif /* KSGPU_H */
