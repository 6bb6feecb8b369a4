// Host-side planning of the assembly path (no device code, no ks_mat): everything ks_mat.hip decides with index arithmetic on the host - the split of
// a row block into its diagonal and ghost parts, the halo plan between the ranks, the binned, windowed and ILU(0) layouts, the plan of the transposed
// product across ranks, MatAXPY on CSR arrays, the sparse LU with fill of KS_PC_LU (ordering, factors, level schedule; tests/test_lu_host.py), the multigrid hierarchy of KS_PC_AMG (tests/test_amg_host.py). Plain functions that fill structs of vectors; constants of the device side come in as parameters and a
// refusal is a status in the result. ks_mat.hip calls a planner and uploads what it filled; KSD_TEST_HOOKS exports each of them as a ksc_* C function,
// and those run on the CPU (tests/test_csr_host.py, test_assembly_host.py, test_sharded_transpose_host.py, test_ilu_host.py, tests/host/assembly_plans.cpp).
#pragma once
#include <vector>

namespace ksc {
// The split of ks_mat_create_csr: a rank's rows with global columns -> the diagonal block (columns the rank owns, as local indices) and the ghost block
// (every other column, as its position in garray, the sorted list of the distinct ghost columns). Both keep the entries of a row in stored order.
// Rows are checked in order, a row's pointer before its columns; the first offence ends the split.
constexpr int SPLIT_ROWPTR = 1, SPLIT_COLUMN = 2;       // rowptr[bad_row + 1] < rowptr[bad_row]; bad_col of bad_row is outside [0, n_global)
struct BlockSplit {
  int status = 0, bad_row = -1, bad_col = 0;
  std::vector<int> rp_d, col_d, rp_o, col_o, garray;
  std::vector<double> val_d, val_o;
};
void csr_split_block(int n_local, int row_start, int n_global, const int *rowptr, const int *col, const double *val, BlockSplit &out);

// The halo plan of the forward product, in the three host steps between its collectives (build_halo_plan, ks_mat.hip). Rank p owns rows
// starts[p] .. starts[p + 1] - 1 (starts has size + 1 entries; a rank may own none).
//   halo_recv_counts  recv_cnt[p] = how many of the sorted ghosts rank p owns (a ghost goes to the LAST rank whose range starts at or below it,
//                     i.e. past the ranks without rows). Every rank then learns every rank's counts: all_cnt, row p = rank p's recv_cnt.
//   halo_peers        the ranks this one exchanges with (ascending; either count non-zero), what it receives from and sends to each, and the
//                     offsets of those segments in the ghost array and the send buffer. Every rank then sends its ghost segments (global ids) to
//                     their owners and receives the ids it has to serve, laid out by send_off / send_cnt.
//   halo_localize_send_idx  those ids as local rows, in place.
constexpr int HALO_UNORDERED = 1, HALO_SELF = 2, HALO_NOT_OWNED = 3;      // starts not ascending; a ghost inside the rank's own range; a served id outside it
int halo_recv_counts(const std::vector<int> &garray, const std::vector<int> &starts, int rank, std::vector<int> &recv_cnt);
struct HaloPeers { std::vector<int> peers, recv_cnt, send_cnt, recv_off, send_off; int nsend = 0; };
void halo_peers(int rank, int size, const int *recv_cnt, const int *all_cnt, HaloPeers &out);
int halo_localize_send_idx(int row_start, int n, int nsend, int *sidx);

// The binned layout (KS_MAT_LAYOUT_BINNED; the kernels that walk it: k_binned_gather, k_binned_reduce, ks_spmv.hip).
// Geometry: ns slices of cs columns - a multiple of the CU count (a workgroup per slice, one resident per CU), each at most cs_max columns - and
// wb = 4 ns wave-bins of wr rows. status: BINNED_16BIT when a column inside its slice or a row inside its wave-bin (wr is the spare accumulator's
// index) does not fit 16 bits, BINNED_32BIT when the padded entries may not fit 32-bit positions.
constexpr int BINNED_16BIT = 1, BINNED_32BIT = 2, BINNED_ORDERS = 3;
struct BinnedGeometry { int status = 0, ns = 0, cs = 0, wb = 0, wr = 0; };
void binned_geometry(int n, long long nnz, int ncu, int cs_max, int seg_pad, BinnedGeometry &out);
// Plan: segment (b, s) holds the entries of wave-bin b's rows with a column in slice s, in stored order, padded to a multiple of seg_pad entries
// (padding: value 0 into row wr, column 0 of the slice). Two orders of the same segments:
//   slice-major (phase 1 reads col16 in it): slice s starts at sbase[s], its segment b at off1[s][b] inside it ([ns][wb + 1]; [wb]: the slice's entries);
//               wseg[s][w] is the segment that holds entry 1024 w of slice s ([ns][nwin]).
//   bin-major, grouped (phase 1 writes G, phase 2 reads G, val2, row16 in it): segment (b, s) starts at off2[b][s] = off2t[s][b]; up to 64 consecutive
//               wave-bins are interleaved slice by slice - [group][slice][wave-bin of the group] - so that what a slice's workgroup writes for a group
//               is one contiguous run. log2[b][s] is the segment's start in wave-bin b's own, logical, stream ([wb][ns + 1]; [ns]: the wave-bin's entries).
// status: BINNED_ORDERS when the two orders do not hold the same number of entries (sbase[ns] against entries).
struct BinnedPlan {
  int status = 0, nwin = 1; long long entries = 0;
  std::vector<unsigned short> col16, row16; std::vector<double> val2;
  std::vector<int> off1, off2t, wseg, off2, log2; std::vector<long long> sbase;
};
void binned_plan(int n, const int *rp, const int *col, const double *val, const BinnedGeometry &g, int seg_pad, BinnedPlan &out);
// what the two kernels do with the plan, on the host. Phase 1: slice by slice, window by window from wseg, G[e + off2t - off1] = x_slice[col16[e]];
// phase 2: wave-bin by wave-bin, its ns pieces through log2 / off2, acc[row16] += val2 * G with acc[wr] the spare, y = acc[0 .. wr).
// The kernel adds by LDS atomics in an order of its own: this walk says nothing about floating-point order and is for checks with exact (integer) sums only.
void binned_apply_host(const BinnedPlan &p, const BinnedGeometry &g, int n, const double *x, double *y);


// P = A + alpha * B on CSR arrays of the same row block (global column indices): MatDuplicate + MatAXPY(P, alpha, B, DIFFERENT_NONZERO_PATTERN),
// the way STMatMAXPY_Private assembles A - sigma B in ST_MATMODE_COPY (src/sys/classes/st/interface/stsolve.c:611-626). rpb == nullptr: B = I
// (MatShift, the nmat = 1 branch, stsolve.c:625), the diagonal of row r being global column row_start + r.
// Entry by entry p_ij = a_ij + (alpha * b_ij) (two roundings: the scaled entry is added as a value of its own), alpha * b_ij where only B has the
// entry, a_ij where only A has it. Rows whose columns ascend strictly in both operands are merged and come out sorted (PETSc's AIJ rows always
// are); a row that is not (repeated or unordered columns, which ks_mat_create_csr accepts) keeps A's entries as they stand, an entry of B going
// to the first entry of A with its column, or to the end of the row. Returns false (nothing built) when the result has more than 2^31 - 1 entries.
bool csr_axpy(int n, int row_start, const int *rpa, const int *ca, const double *va, double alpha, const int *rpb, const int *cb, const double *vb,
              std::vector<int> &rp, std::vector<int> &col, std::vector<double> &val);
// B = A^T for a CSR block of nrows x ncols (MatTranspose, MAT_INITIAL_MATRIX): a counting sort by column; the rows of B list their entries in
// ascending row order of A (sorted columns out whatever the order inside A's rows; repeated entries of A stay separate entries).
void csr_transpose(int nrows, int ncols, const int *rp, const int *col, const double *val, std::vector<int> &rpt, std::vector<int> &colt, std::vector<double> &valt);

// The plan of y = A^T x for a row-sharded A (KS_MAT_SHARDED_TRANSPOSE), rank by rank and without communication: MatMultTranspose_MPIAIJ's three
// steps on this library's halo plan. From the rank's rows (global columns), its sorted ghost list (the distinct columns other ranks own) and
// send_idx (the local rows it packs for its peers in a forward product, peer after peer in ascending rank):
//   d_*    the transposed DIAGONAL block (entries whose column this rank owns), n x n with local indices, by the counting sort of csr_transpose:
//          row c lists the entries of column c by ascending original row, duplicates in their original order.
//   o_*    the transposed OFF-DIAGONAL block, a CSR of nghost rows: row g lists the local rows of A that hold ghost column g (ascending, stable)
//          with their values. o_rp * x[o_row] summed per row is what the owner of ghost g has to add to its y.
//   acc_*  the inverse of send_idx. The reverse exchange delivers, at position e of the receive buffer, a peer's sum for local row send_idx[e].
//          acc_rows: the distinct local rows any peer reads, ascending; acc_pos[acc_ptr[i] .. acc_ptr[i+1]) the positions of row acc_rows[i],
//          ascending - and so by ascending peer rank, the buffer being ordered by peer. acc_pos is a permutation of 0 .. nsend-1.
struct ShardedTransposePlan {
  std::vector<int> d_rp, d_col; std::vector<double> d_val;
  std::vector<int> o_rp, o_row; std::vector<double> o_val;
  std::vector<int> acc_rows, acc_ptr, acc_pos;
};
void sharded_transpose_plan(int n, int row_start, const int *rp, const int *col, const double *val, int nghost, const int *ghosts,
                            int nsend, const int *send_idx, ShardedTransposePlan &out);
// what the device runs, on the host, for one rank: rsend[g] = sum of o_val * x[o_row] over ghost row g (fma, stored order) and y = (diagonal block)^T x
// (fma, stored order); then, once the exchange has filled rrecv, y[acc_rows[i]] += rrecv[pos] over the row's positions in ascending order
void sharded_transpose_local_host(const ShardedTransposePlan &p, int n, int nghost, const double *x, double *rsend, double *y);
void sharded_transpose_add_host(const ShardedTransposePlan &p, const double *rrecv, double *y);

// The plan of the windowed CSR layout (KS_MAT_LAYOUT_WINDOW; the kernel that walks it: k_spmv_window, ks_spmv.hip). Rows are cut into blocks of
// block_rows; a block lists, ascending, the 64-double segments of x (col >> 6) its entries reference. With at most max_segments of them it is a
// WINDOW block: its entries keep one 16-bit code each, slot * 64 + (col & 63), slot being the segment's position in the block's list. With more
// it is a DIRECT block: it keeps its 32-bit columns in `dcol`, entry e of the CSR stream at dcol[dbase[block] + e]; dbase is a multiple of four,
// so a load that is aligned in the CSR stream is aligned in dcol too (the gaps that costs hold column 0). Everything is in CSR entry order.
constexpr int WIN_NOT_DIRECT = -2147483647 - 1;         // dbase of a window block
struct WindowPlan {
  long long blocks = 0, direct_blocks = 0, window_entries = 0, direct_entries = 0, total_segments = 0;
  std::vector<int> nseg;                  // [blocks] segments a block references (window and direct blocks alike)
  std::vector<int> segptr, seg;           // [blocks + 1], [total_segments]: the lists of the window blocks (a direct block's list is empty)
  std::vector<int> dbase;                 // [blocks]
  std::vector<unsigned short> codes;      // [nnz + pad], 0 at the entries of direct blocks
  std::vector<int> dcol;                  // [entries of direct blocks + gaps + pad]
};
// pad: what the code and column arrays are longer than their last entry (CW_PAD)
void csr_window_plan(int n, const int *rp, const int *col, int block_rows, int max_segments, int pad, WindowPlan &out);

// Block CSR (BAIJ) input, ks_mat_create_bsr. A rank's nb block rows of bs x bs blocks: browptr (nb + 1), bcol (GLOBAL block columns, any order, repeats
// allowed), bval (block k column-major at bval + k bs bs, as PETSc's Mat_SeqBAIJ::a).
//   bsr_expand  the CSR arrays that define the matrix: scalar row bs I + i holds, for each block k of block row I in stored order and then c = 0 .. bs - 1,
//               the entry (bs bcol[k] + c, blk_k(i, c)); explicit zeros inside blocks are entries. Checked first, in this order: every row pointer
//               (BSR_ROWPTR: browptr[bad_row + 1] < browptr[bad_row]), the size (BSR_TOO_LARGE: more than 2^31 - 1 stored scalars; nothing of bcol has
//               been read by then), every block column in block row order (BSR_COLUMN: bad_col of block row bad_row is outside [0, nb_global)). On a
//               status nothing is filled.
constexpr int BSR_ROWPTR = 1, BSR_COLUMN = 2, BSR_TOO_LARGE = 3;
struct BsrExpansion { int status = 0, bad_row = -1, bad_col = 0; std::vector<int> rp, col; std::vector<double> val; };
void bsr_expand(int bs, int nb, int nb_global, const int *browptr, const int *bcol, const double *bval, BsrExpansion &out);
//   bsr_diag    the blocks of the rank's own block columns [bstart, bstart + nb), with local block columns and in stored order: the diagonal block of
//               the expansion's split (csr_split_block), block by block.
//   bsr_plan    the device image of those (KS_MAT_LAYOUT_BSR; the kernels that walk it: k_spmv_bsr, k_spmm_bsr). val holds every block ROW-major - the lane
//               of scalar row i reads blk(i, 0 .. bs - 1) as one contiguous run - block after block in stored order, and is `pad` scalars longer than
//               its last block, as bcol is `pad` blocks longer (the CW_PAD rule: what a chunk load may read past the end; zeros). A workgroup takes
//               group_rows consecutive block rows per step, wave w of it wave_rows = group_rows / 4 of them; gptr (groups + 1) are the groups' bounds
//               in the block stream, gptr[g] = browptr[min(g group_rows, nb)].
struct BsrBlocks { std::vector<int> browptr, bcol; std::vector<double> bval; };       // bval as given: column-major blocks
void bsr_diag(int bs, int nb, int bstart, const int *browptr, const int *bcol, const double *bval, BsrBlocks &out);
struct BsrPlan { int bs = 0, nb = 0, group_rows = 0, chunk_blocks = 0; long long blocks = 0, groups = 0; std::vector<int> browptr, bcol, gptr; std::vector<double> val; };
void bsr_plan(int bs, int nb, const int *browptr, const int *bcol, const double *bval, int group_rows, int chunk_blocks, int pad, BsrPlan &out);
// the kernel's walk on the host: group by group, wave by wave, the wave's run of blocks in chunks of chunk_blocks; inside a chunk scalar row i of a block
// row runs acc = fma(blk(i, c), x[bs bcol + c], acc) over its blocks of the chunk in stored order, c ascending - from 0.0: the entry order of the expansion
void bsr_apply_host(const BsrPlan &p, const double *x, double *y);

// ILU(0) of the diagonal blocks of a CSR row block, laid out for k_bjacobi_ilu_apply (ks_pc.hip): PCBJACOBI with -sub_pc_type ilu at zero fill
// (PETSc's MatILUFactorSymbolic/Numeric on each block, natural ordering). Block b is local rows b*bs .. min(n, (b+1)*bs) - 1 and the columns
// row_start + the same range; everything else in those rows (other blocks, ghost columns) is dropped. A block's rows are sorted by column and
// repeated entries summed in the order they are stored; the sorted pattern (explicit zeros included) is factored in place in IKJ order, no
// pivoting, no fill: l_ik = a_ik / u_kk, a_ij -= l_ik u_kj for the j > k of row k that row i stores. L is unit lower triangular.
// The solves run level by level: a row's level is one more than the largest level among the rows it reads (L: the columns left of the diagonal,
// levels ascending from row 0; U: the columns right of it, ascending from the last row). Per block the rows are listed by level (ascending row
// inside a level), first the L levels, then the U levels, and a level's off-diagonal entries are stored slot-major across its rows - ELL per
// level, padded to the level's longest row: entry s of the row at position p of a level of nl rows is at (level's start) + s * nl + p. A code
// is the entry's block-local column; padding is a zero value with the row's own index as its code (an entry that reads nothing new).
struct IluBlock { long long ell; int lev, nL, nU, pad; };      // where the block's entries and level descriptors start; its numbers of L and U levels
struct IluPlan {
  int status = 0, bad_block = -1, bad_row = -1;   // 0, or ILU_NO_DIAGONAL / ILU_ZERO_PIVOT with the block and the local row
  int longest_row = 0;                            // most entries in one row of a block, diagonal included
  std::vector<IluBlock> blk;                      // [blocks]
  std::vector<int> lev;                           // two per level: rows, slots (a block's L levels, then its U levels)
  std::vector<double> val;                        // ELL values of every level
  std::vector<unsigned short> code;               // their block-local columns
  std::vector<unsigned short> rows;               // [2 n]: block b's rows in L level order at 2 * b * bs, in U level order behind them
  std::vector<double> dinv;                       // [n]: 1 / u_rr in the block's U level order (position p of the U list at b * bs + p)
  std::vector<int> frp, fcol; std::vector<double> fval;   // the factors on the blocks' sorted patterns (block-local columns), kept only on request
};
constexpr int ILU_NO_DIAGONAL = 1, ILU_ZERO_PIVOT = 2;
constexpr int ILU_BS_MAX = 8192;                  // 64 KB of LDS for the block's vector; codes fit 16 bits
// tr (optional): a second plan of the same factors for the transposed solve y = (LU)^-T x = L^-T U^-T x (PCApplyTranspose; k_bjacobi_ilu_apply_t). It is
// NOT an ILU(0) of the transposed block. Block by block the factors are transposed by a counting sort, so row r of U^T lists column r of U in
// ascending original row, and the level sets are recomputed for the transposed triangles (as many levels as the forward solve, other members).
// The layout is the same; what differs: the FIRST run of levels (nL of the block record) is U^T - lower triangular, with the pivots - and the
// second (nU) is L^T, unit upper; dinv is 1 / u_rr in the first run's level order; longest_row is the longest column of a block.
void csr_ilu0_blocks(int n, int row_start, int bs, const int *rp, const int *col, const double *val, bool keep_factors, IluPlan &out, IluPlan *tr = nullptr);
// what the kernels compute, on the host, in the same order: out = (LU)^-1 in block by block from the forward plan, out = (LU)^-T in from the transposed one
void ilu0_apply_host(const IluPlan &p, int n, int bs, const double *in, double *out);
void ilu0_apply_transpose_host(const IluPlan &t, int n, int bs, const double *in, double *out);

// Sparse LU with fill of a whole square matrix (KS_PC_LU; the kernels that walk the plan: ks_pc_lu.hip): PCLU with PETSc's defaults - a nested
// dissection ordering applied symmetrically, no pivoting - Q P Q^T = L U, L unit lower triangular. The rows of P are sorted by column and repeated
// entries summed in stored order, as for the ILU(0) blocks; the diagonal position is always part of the pattern (an absent diagonal entry is a
// structural zero that fill may make non-zero). Columns outside [0, n) are ignored (one rank owns every row).
//   ordering   lu_ordering: the graph of the pattern of P + P^T. LU_ORDERING_ND is George's automatic nested dissection on rooted level
//              structures: per connected component, start from the smallest node; up to five times take as the new root the node of the last
//              level with the fewest neighbours inside the component (lowest index on ties) while the structure gets deeper; the middle level
//              (levels / 2) is the separator; what is left is ordered the same way, the separator (ascending) goes last. Components of at most
//              8 nodes or with fewer than 3 levels are listed ascending. perm[i] = the original row eliminated i-th. Deterministic.
//   factors    row by row in IKJ order: the pattern of row i is the union of its own entries and the U patterns of the rows k of its L part,
//              taken ascending (fill included); l_ik = a_ik / u_kk, a_ij -= l_ik u_kj, one rounding per operation. No entry of the pattern is
//              dropped, whatever its value. u_ii == 0 ends the factorisation: status LU_ZERO_PIVOT, bad_row = the ORIGINAL row.
//   levels     of the two triangles as for the ILU(0) blocks: a row's level is one more than the largest level among the rows it reads.
//   layout     the rows of the triangle solved first at positions [0, n) and of the one solved second at [n, 2n), in level order (ascending row
//              inside a level); rp (2n + 1) points into col / val, where a row's off-diagonal entries are contiguous with ascending column
//              (permuted numbering). lev (levels + 1) are the positions where the levels start, the first triangle's levels first.
//              dinv is 1 / u_rr in the level order of the triangle that carries the pivots (first_scaled: the first one - the transposed plan).
//   stages     the levels of each triangle cut in order into runs: a WIDE stage is a run of levels with at least `wide` rows each (one launch
//              per level, lanes[level] = 1, 8 or 64 lanes per row by the level's mean row length), a NARROW stage a maximal run of levels with
//              fewer (one launch of one workgroup, a wave of 64 lanes per row).
constexpr int LU_ORDERING_ND = 0, LU_ORDERING_NATURAL = 1;
constexpr int LU_ZERO_PIVOT = 1, LU_TOO_LARGE = 2;        // LU_TOO_LARGE: more than 2^31 - 1 stored entries in the factors
struct LuStage { int lev0, nlev, wide; };
struct LuPlan {
  int status = 0, bad_row = -1;
  int n = 0, longest_row = 0;                     // longest_row: most entries in one row of L + U, diagonal included
  long long nnzL = 0, nnzU = 0;                   // stored entries of L (without the unit diagonal) and of U (with the diagonal)
  int levels[2] = {0, 0}, nstage[2] = {0, 0};     // of the triangle solved first and of the one solved second
  int first_scaled = 0;                           // 0: L then U (forward), 1: U^T then L^T (transposed)
  int wide = 0, neg = 0, pos = 0;                 // the threshold the stages were cut with; signs of the pivots u_rr
  std::vector<int> perm, rows, rp, col, lev, lanes;
  std::vector<double> val, dinv;
  std::vector<LuStage> stages;
  std::vector<int> lrp, lcol, urp, ucol; std::vector<double> lval, uval;      // the factors by rows in permuted numbering (U rows start with the pivot), kept only on request
};
void lu_ordering(int n, const int *rp, const int *col, int ordering, std::vector<int> &perm);
// tr (optional): a second plan of the SAME factors for y = Q^T L^-T U^-T Q x, made the way csr_ilu0_blocks makes its transposed plan
void csr_lu_plan(int n, const int *rp, const int *col, const double *val, int ordering, int wide, bool keep_factors, LuPlan &out, LuPlan *tr = nullptr);
// what the kernels compute, in their summation order: lane l of a row's group takes entries l, l + lanes, ... ascending by fma, the partial sums are
// combined in the fixed order of the wave sums (ks_sweeps.cuh). out = Q^T U^-1 L^-1 Q in from the forward plan, Q^T L^-T U^-T Q in from the transposed
void lu_apply_host(const LuPlan &p, const double *in, double *out);
void lu_apply_transpose_host(const LuPlan &t, const double *in, double *out);

// The hierarchy of the smoothed-aggregation multigrid preconditioner (KS_PC_AMG; the kernels that walk it: ks_pc_amg.hip). Level 0 is P itself, its
// rows sorted by column and repeated entries summed in stored order (columns outside [0, n) ignored: one rank owns every row); explicit zeros stay
// entries. A level that has at most coarse_limit rows, or is the max_levels-th, is the last. Otherwise, in order:
//   diagonal   d_i = a_ii; a row that stores none, or a zero, ends the plan: status AMG_NO_DIAGONAL with the level and the row.
//              rho = max_i (sum_j |a_ij|) / |a_ii|: Gershgorin's bound of the spectral radius of D^-1 A, never an underestimate.
//   strength   the graph with an edge i - j (i != j) when a_ij != 0 and |a_ij| >= theta sqrt(|a_ii a_jj|) or the same holds for a_ji; the edge's
//              weight is max(|a_ij|, |a_ji|), an entry that is not stored counting as 0.
//   aggregates three passes, every loop ascending. 1: an unaggregated node with neighbours, none of them aggregated, founds an aggregate with all
//              of them. 2: a node still outside joins the aggregate of the neighbour with the largest weight among those pass 1 aggregated (what
//              pass 2 assigns is not looked at; ties: the lowest column). 3: a node still outside that has neighbours founds an aggregate with
//              the neighbours still outside. A node without neighbours stays outside (agg = -1): its row of the prolongator is empty.
//              No aggregate at all, or more than `stall` times the rows, makes this level the last.
//   transfer   T has one column per aggregate with the entries 1 / sqrt(size). The prolongator is T, or smoothed P = (I - (4 / (3 rho)) D^-1 A) T:
//              row i sums a_ij t_j by fma in ascending j into its aggregates' columns, then p_ic = t_ic - ((4 / (3 rho)) / d_i) sum_c. The
//              pattern is that of A T joined with T's; nothing is dropped. R = P^T by the counting sort of csr_transpose.
//   Galerkin   A_c = R (A P), both products row by row (Gustavson): the entries of the left row ascending, for each the right row ascending,
//              acc[col] = fma(left, right, acc[col]); a row's columns come out ascending. Nothing is dropped.
// status AMG_TOO_LARGE: a product with more than 2^31 - 1 entries. Deterministic; allocation failures are exceptions of the vectors.
constexpr int AMG_NO_DIAGONAL = 1, AMG_TOO_LARGE = 2;
constexpr int AMG_MAX_LEVELS = 16;
struct AmgOptions { double theta = 0.0; int coarse_limit = 200, max_levels = 10; bool smooth = true; double stall = 0.8; };
struct AmgLevel {
  int n = 0, nagg = 0; double rho = 0.0;                      // rho, dinv, agg and the transfers: every level but the last
  std::vector<int> rp, col; std::vector<double> val;          // the level's operator
  std::vector<double> dinv;                                   // 1 / a_ii
  std::vector<int> agg;                                       // the aggregate of a row, -1: none
  std::vector<int> prp, pcol; std::vector<double> pval;       // P: n x nagg
  std::vector<int> rrp, rcol; std::vector<double> rval;       // R: nagg x n
};
struct AmgPlan { int status = 0, bad_level = -1, bad_row = -1; std::vector<AmgLevel> levels; };
void amg_plan(int n, const int *rp, const int *col, const double *val, const AmgOptions &opt, AmgPlan &out);
}
