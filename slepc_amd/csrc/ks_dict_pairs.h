// The pair form of the dictionary layout's row walk: a lane owns the two consecutive rows r (even) and r + 1 and brings x in with 16-byte loads.
// A row of the row-pattern form reads x[r + o] for the offsets o of its pattern. When every offset is b + d with b even, b itself an offset of the
// dictionary and d in {-1, 0, +1}, the rows r and r + 1 need for a base b the pair x[r + b], x[r + b + 1] (one aligned 16-byte load: r and b are even),
// the element in front of it and the element behind it; those two are the neighbouring lanes' halves of the same load (a one-lane shift), and the first
// and last lane of a wave load them as single elements. Seven 8-byte gathers per row become five 16-byte loads per row pair on the 7-point stencil.
// The fma chain runs over the CANDIDATES (base, d) in ascending order of b + d instead of over the row's entry slots: the plan accepts a matrix only if
// every pattern has its entries in strictly ascending offsets, so the entries of a row meet the chain in the order of the one-row walk
// (ksr::dict_word_row); a candidate the row does not have leaves acc untouched (its fma is computed and dropped by a select: an fma(0.0, 0.0, acc) in
// its place would turn an acc of -0.0, which a product that underflows leaves behind, into +0.0 in the middle of the chain), and a row with fewer than W
// entries ends with the one fma(0.0, 0.0, acc) that the one-row walk's padding slots amount to (bit 31 of the pattern's mask). Same products, same
// order, same padding: same bits, the sign of a zero included. Selecting x
// per entry slot from the loaded registers instead costs a compare and two v_cndmask per candidate and slot - more instructions than the gathers it saves.
// Eligibility (dict_pair_plan): the bases are the even offsets of the dictionary itself - a pair no row of the matrix reads is never loaded, so an odd
// stride (offsets +-301: no even offset next to them) keeps the one-row walk - at most 9 of them; an odd offset between two bases 2 apart is the lower one's.
// No address outside [x, x + n) is loaded: every load is bounded by its own elements, not by the row (pair_ld below).
// Plain C++ apart from KS_PAIR_HD: the host test compiles this file alone and emulates a wave with a loop (the Lane argument is the loads and the lane shift).
#pragma once
#include <cmath>
#include <cstring>
#include <vector>
#include <algorithm>

#if defined(__HIPCC__)
#define KS_PAIR_HD __host__ __device__ __forceinline__
#define KS_PAIR_UNROLL _Pragma("unroll")
#define KS_PAIR_NOUNROLL _Pragma("unroll 1")
#else
#define KS_PAIR_HD inline
#define KS_PAIR_UNROLL
#define KS_PAIR_NOUNROLL
#endif

namespace ksp {

constexpr int PAIR_MAX_BASES = 9;              // 5-point: 3, 7-point: 5, 27-point: 9
constexpr int PAIR_MAX_TABLE = 2048;           // doubles of the coefficient table in LDS (npat * 3 * nb): 16 KB

// what the kernels take by value (uniform: it stays in scalar registers)
struct PairArgs {
  int nb = 0;                                  // bases, ascending
  unsigned dmask = 0;                          // bit k: base k has a candidate with d != 0
  int base[PAIR_MAX_BASES] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
};

// The plan, decided once at assembly from the host copies of the dictionaries and the pattern table (pure host).
struct PairPlan {
  bool ok = false; const char *why = "";
  PairArgs args;
  std::vector<double> coef;                    // [npat][3 nb]: the value of the pattern's entry at candidate 3 k + d + 1, 0.0 where it has none
  std::vector<unsigned> mask;                  // [npat]: bit 3 k + d + 1 set where the pattern has that entry; bit 31: the pattern has padding slots (fewer than W entries)
};
// pats: npat words of W 2-byte codes (offset code | value code << 8, value code 255 = padding), null when the matrix is not in the row-pattern form
static inline PairPlan dict_pair_plan(int W, int npat, const unsigned short *pats, const int *offs, int noff, const double *vals, int nval)
{
  PairPlan P;
  auto no = [&](const char *why) { P.ok = false; P.why = why; return P; };
  if (!pats || npat <= 0) return no("not in the row-pattern form");
  if (W != 8 && W != 16 && W != 32) return no("W is none of 8, 16, 32");
  std::vector<int> bases;
  for (int i = 0; i < noff; i++) if (offs[i] % 2 == 0) bases.push_back(offs[i]);
  std::sort(bases.begin(), bases.end());
  if (bases.empty()) return no("no even offset");
  if ((int)bases.size() > PAIR_MAX_BASES) return no("more than 9 bases");
  const int nb = (int)bases.size();
  std::vector<int> cand(noff, -1);             // offset code -> candidate
  for (int i = 0; i < noff; i++) {
    const int o = offs[i];
    for (int k = nb - 1; k >= 0; k--) if (o >= bases[k] - 1 && o <= bases[k] + 1) cand[i] = 3 * k + (o - bases[k]) + 1;     // between two bases 2 apart: the lower one's
    if (cand[i] < 0) return no("an offset is not within 1 of an even offset of the dictionary");
    if (o != bases[cand[i] / 3]) P.args.dmask |= 1u << (cand[i] / 3);
  }
  if ((long long)npat * 3 * nb > PAIR_MAX_TABLE) return no("coefficient table too large");
  P.args.nb = nb;
  for (int k = 0; k < nb; k++) P.args.base[k] = bases[k];
  P.coef.assign((size_t)npat * 3 * nb, 0.0); P.mask.assign(npat, 0u);
  for (int p = 0; p < npat; p++) {
    long long last = -(1LL << 40);
    int entries = 0;
    for (int e = 0; e < W; e++) {
      const unsigned code = pats[(size_t)p * W + e], oc = code & 255u, vc = code >> 8;
      if (vc == 255u) continue;                                       // padding: fma(0.0, 0.0, acc) wherever it stands
      if ((int)oc >= noff || (int)vc >= nval) return no("a code outside its dictionary");
      if (offs[oc] <= last) return no("a pattern's entries are not in ascending offsets");
      last = offs[oc];
      P.coef[(size_t)p * 3 * nb + cand[oc]] = vals[vc];
      P.mask[p] |= 1u << cand[oc];
      entries++;
    }
    if (entries < W) P.mask[p] |= 1u << 31;
  }
  P.ok = true; P.why = "";
  return P;
}

struct D2 { double x, y; };
// The rule of every load of x in the walk, written out for the host: x[i], x[i + 1] with i even is one 16-byte load when both lie in [0, n); an element
// outside counts as 0.0 and is never loaded (x must be 16-byte aligned). On the device the same rule is the hardware's: ksr::PairLane loads through a
// buffer descriptor of exactly [x, x + n), whose range check answers 0.0 for what lies outside without a memory access and without a branch.
inline D2 pair_ld(const double *x, long long n, long long i)
{
  D2 v = {0.0, 0.0};
  if (i >= 0 && i + 1 < n) std::memcpy(&v, x + i, 16);
  else if (i >= 0 && i < n) v.x = x[i];                               // odd n: the last element on its own
  return v;
}
inline double one_ld(const double *x, long long n, long long i, bool want) { return want && i >= 0 && i < n ? x[i] : 0.0; }

// One row of the row-pattern form straight from the tables in memory, entry by entry: the chain of the one-row walk (ksr::dict_word_row). For the single
// row a pair kernel has behind its last pair when n is odd: nothing there is worth registers or LDS. W is the matrix's own (the stride of pats).
template <int W>
KS_PAIR_HD double dict_row_from_tables(const unsigned char *rowpat, const unsigned short *pats, long long r, const double *dval, const int *doff, const double *x)
{
  const int p = rowpat[r];
  double acc = 0.0;
KS_PAIR_NOUNROLL
  for (int e = 0; e < W; e++) {
    const unsigned code = pats[p * W + e], oc = code & 0xffu, vc = code >> 8;
    const bool ok = vc != 255u;
    acc = fma(ok ? dval[vc] : 0.0, ok ? x[r + doff[oc]] : 0.0, acc);
  }
  return acc;
}

// one candidate of a row's chain: acc = fma(a, x, acc) where the pattern has the entry (bit of its mask), acc as it is where not
KS_PAIR_HD double pair_step(double acc, double a, double x, unsigned mask, int bit) { const double t = fma(a, x, acc); return mask >> bit & 1u ? t : acc; }

// rows r and r + 1 of patterns p0 and p1 (r even; a lane without rows passes any valid pattern and drops the results: its loads serve its neighbours).
// coef, mask: the plan's tables (the kernels keep them in LDS). NBT: compiled number of bases, >= pa.nb. Lane: how this lane reaches x and its neighbours -
// lane(), pair(i) and one(i, want) under the rule above, up(v, i): the value v of the lane below (i: the index this lane loaded v from, for the host
// emulation, which has no wave), down(v, i): of the lane above. Every lane of the wave must call this together.
// The walk in its two halves, for a caller that asks for the loads in another way (the pipelined forward update, ks_gs.hip): dict_pair_loads fills v[k] = x[r + b_k],
// x[r + b_k + 1] and, for a wide base, edge[k] = x[r + b_k - 1] in the wave's first lane, x[r + b_k + 2] in its last (set and read only under the same uniform
// conditions); dict_pair_sums is every row's chain over them. dict_pair_walk is the one after the other.
template <int NBT, class Lane>
KS_PAIR_HD void dict_pair_loads(const PairArgs &pa, long long r, const Lane &ln, D2 (&v)[NBT], double (&edge)[NBT])
{
  static_assert(NBT >= 1 && NBT <= PAIR_MAX_BASES, "compiled bases");
  const int lane = ln.lane();
KS_PAIR_UNROLL
  for (int k = 0; k < NBT; k++) {                                     // every load first: nothing below waits for one base before the next is asked for
    if (k < pa.nb) {
      const long long i = r + pa.base[k];
      v[k] = ln.pair(i);
      if (pa.dmask >> k & 1u) edge[k] = ln.one(lane == 0 ? i - 1 : i + 2, lane == 0 || lane == 63);      // the wave's first and last lane have no neighbour to take these from: one load serves both
    }
  }
}
template <int NBT, class Lane>
KS_PAIR_HD void dict_pair_sums(const PairArgs &pa, const double *coef, const unsigned *mask, int p0, int p1, long long r, const Lane &ln, const D2 (&v)[NBT], const double (&edge)[NBT], double &y0, double &y1)
{
  const int lane = ln.lane();
  const int stride = 3 * pa.nb;
  const double *c0 = coef + p0 * stride, *c1 = coef + p1 * stride;
  const unsigned m0 = mask[p0], m1 = mask[p1];
  double a0 = 0.0, a1 = 0.0;
KS_PAIR_UNROLL
  for (int k = 0; k < NBT; k++) {
    if (k < pa.nb) {
      const D2 x0 = v[k];
      if (pa.dmask >> k & 1u) {                                       // the three candidates of a wide base, each row's chain in ascending offsets
        const long long i = r + pa.base[k];
        const double below = ln.up(x0.y, i), above = ln.down(x0.x, i);
        const double lo = lane == 0 ? edge[k] : below, hi = lane == 63 ? edge[k] : above;      // x[r + b - 1], x[r + b + 2]
        a0 = pair_step(a0, c0[3 * k], lo, m0, 3 * k);
        a0 = pair_step(a0, c0[3 * k + 1], x0.x, m0, 3 * k + 1);
        a0 = pair_step(a0, c0[3 * k + 2], x0.y, m0, 3 * k + 2);
        a1 = pair_step(a1, c1[3 * k], x0.x, m1, 3 * k);
        a1 = pair_step(a1, c1[3 * k + 1], x0.y, m1, 3 * k + 1);
        a1 = pair_step(a1, c1[3 * k + 2], hi, m1, 3 * k + 2);
      } else {
        a0 = pair_step(a0, c0[3 * k + 1], x0.x, m0, 3 * k + 1);
        a1 = pair_step(a1, c1[3 * k + 1], x0.y, m1, 3 * k + 1);
      }
    }
  }
  a0 = pair_step(a0, 0.0, 0.0, m0, 31);                               // the padding slots of the one-row walk
  a1 = pair_step(a1, 0.0, 0.0, m1, 31);
  y0 = a0; y1 = a1;
}
template <int NBT, class Lane>
KS_PAIR_HD void dict_pair_walk(const PairArgs &pa, const double *coef, const unsigned *mask, int p0, int p1, long long r, const Lane &ln, double &y0, double &y1)
{
  D2 v[NBT]; double edge[NBT];
  dict_pair_loads<NBT>(pa, r, ln, v, edge);
  dict_pair_sums<NBT>(pa, coef, mask, p0, p1, r, ln, v, edge, y0, y1);
}

} // namespace ksp
