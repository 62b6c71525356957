// Minimizer runs of one read as a bit set of minimizer positions (k_scan's mask
// path), shared by the kernel and the CPU check program
// (tools/mg_runs_check_main.cpp).
//
// The minimizer positions of a read's successive windows j = 1 .. J (window j =
// m-mers [j, j + w - 1]) never decrease, so the read's runs are the set bits of
//   P: bit x = p + m set iff m-mer position p is the minimizer of some window,
// in order, and the windows of each run follow from its successor alone
// (run_end): the next minimizer either takes over the moment it enters the
// window (its key is smaller: the run ends at window p' - w) or waits until the
// current one leaves (the run ends at window p).  Keys are order key | position,
// so an equal order key never takes over: leftmost on ties.  The first run
// opens at window 1, every other one after its predecessor, the last ends at J.
// The bit index is shifted by m so that the step at m-mer position t touches
// chunk (t + m) >> 5 -- the read word whose base the step rolls in -- and the
// chunk before it (w <= 33).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MG_RUNS_HD __host__ __device__ __forceinline__
#else
#define MG_RUNS_HD inline
#endif

namespace mg_runs {

// Set bit s of the chunk pair (lo = chunk k - 1, hi = chunk k), s counted from
// bit 0 of lo.  Only s mod 64 is used, so the caller may leave a key's high bits
// on a position; a caller whose position fell behind the pair (a lane past its
// read, which holds its last position) sets a bit above that position, which
// clip() removes.
MG_RUNS_HD void mark(uint32_t& lo, uint32_t& hi, uint32_t s) {
  const uint64_t b = 1ull << (s & 63u);
  lo |= (uint32_t)b;
  hi |= (uint32_t)(b >> 32);
}

// Keep the bits x <= X of a valid read, nothing of a read without windows.
template <int N>
MG_RUNS_HD void clip(uint32_t (&c)[N], int X, bool valid) {
  const int xc = X >> 5;
  const uint32_t part = 0xFFFFFFFFu >> (31 - (X & 31));
#pragma unroll
  for (int k = 0; k < N; ++k) c[k] = (!valid || k > xc) ? 0u : (k == xc ? c[k] & part : c[k]);
}

template <int N>
MG_RUNS_HD uint32_t count(const uint32_t (&c)[N]) {
  uint32_t n = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) n += (uint32_t)__builtin_popcount(c[k]);
  return n;
}

// Drop an empty lowest chunk: chunk k + 1 moves to k and base advances by 32.
// carry(s) moves whatever travels with the chunks (the kernel's read words).
template <int N, class F>
MG_RUNS_HD void shift(uint32_t (&c)[N], int& base, F&& carry) {
  const bool s = c[0] == 0;
#pragma unroll
  for (int k = 0; k + 1 < N; ++k) c[k] = s ? c[k + 1] : c[k];
  c[N - 1] = s ? 0u : c[N - 1];
  base += s ? 32 : 0;
  carry(s);
}

// Take the lowest set bit: its index, base included.  One shift first, plus
// EXTRA more: EXTRA = 0 serves a set whose successive bits lie at most 32 apart
// once the leading empty chunks are gone (successive minimizers are at most w
// apart: w <= 32).  An empty set returns base + 31 and stays empty.
template <int N, int EXTRA, class F>
MG_RUNS_HD int pop(uint32_t (&c)[N], int& base, F&& carry) {
#pragma unroll
  for (int e = 0; e <= EXTRA; ++e) shift<N>(c, base, carry);
  const uint32_t v = c[0];
  const int b = __builtin_ctz(v | 0x80000000u);
  c[0] = v & (v - 1u);
  return base + b;
}

struct NoCarry {
  MG_RUNS_HD void operator()(bool) const {}
};

// Last window of the run of minimizer p (key = order key | p) whose successor
// is pn (keyn); last: the read's last run.
MG_RUNS_HD int run_end(int p, uint32_t key, int pn, uint32_t keyn, bool last, int J, int w) {
  return last ? J : (keyn < key ? pn - w : p);
}

// Run i of P: position p and window range [lo, hi]; key_at(p) = order key | p
// of the m-mer at p.  false: no such run.
template <int N, class K>
MG_RUNS_HD bool decode(const uint32_t (&P0)[N], int J, int m, int w, uint32_t i, K&& key_at, int& p, int& lo, int& hi) {
  uint32_t P[N];
  for (int k = 0; k < N; ++k) P[k] = P0[k];
  const uint32_t n = count<N>(P);
  if (i >= n) return false;
  int xb = 0;
  int pc = pop<N, N - 1>(P, xb, NoCarry()) - m;
  lo = 1;
  for (uint32_t r = 0;; ++r) {
    const int pn = pop<N, N - 1>(P, xb, NoCarry()) - m;
    const bool last = r + 1 == n;
    hi = run_end(pc, key_at(pc), pn, last ? 0u : key_at(pn), last, J, w);
    if (r == i) break;
    lo = hi + 1;
    pc = pn;
  }
  p = pc;
  return true;
}

}  // namespace mg_runs
