// mg_runs_check — a stand-alone host check of the run bit set (device/mg_runs.hpp,
// the helpers k_scan's mask path shares), meant to be built with
// -fsanitize=address,undefined (make runs_check_asan) and run on the CPU.  It
// takes no arguments.  For random and adversarial order-key sequences it
// records a read's minimizer positions twice -- by the definition (one bit per
// position) and, for w <= 32, the way the kernel does (one loop per read word,
// mg_runs::mark on the chunk pair of that word with the key's high bits left
// on, an unguarded phase up to some step every lane reaches, then lanes past
// their read holding their last minimum up to the end of a longer read's
// loop, mg_runs::clip, the leading shifts, the emission one run behind its
// successor) -- decodes them with mg_runs::pop / run_end / decode and compares
// every (p, jlo, jhi) with a brute-force minimum of (order key | position) per
// window, leftmost on ties.
// Exit status 0 = all checks passed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "mg_runs.hpp"

namespace {

struct Run {
  int p, lo, hi;
  bool operator==(const Run& o) const { return p == o.p && lo == o.lo && hi == o.hi; }
};

long g_cases = 0, g_runs = 0;

int fail(const std::string& what, int n, int m, int w) {
  std::fprintf(stderr, "mg_runs_check: FAILED: %s (n = %d, m = %d, w = %d)\n", what.c_str(), n, m, w);
  return 1;
}

// windows j = 1 .. J of m-mers [j, j + w - 1]; key[t] for t = 0 .. n - m
std::vector<Run> brute(const std::vector<uint32_t>& key, int J, int w) {
  std::vector<Run> r;
  for (int j = 1; j <= J; ++j) {
    int best = j;
    for (int t = j + 1; t <= j + w - 1; ++t)
      if (key[t] < key[best]) best = t;
    if (r.empty() || r.back().p != best)
      r.push_back({best, j, j});
    else
      r.back().hi = j;
  }
  return r;
}

// minimizer position of the window that ends at m-mer t (t >= w)
int window_min(const std::vector<uint32_t>& key, int t, int w) {
  int best = t - w + 1;
  for (int s = best + 1; s <= t; ++s)
    if (key[s] < key[best]) best = s;
  return best;
}

template <int N>
int check(const std::vector<uint32_t>& key, int n, int m, int w, int tmax_extra, int tall_back) {
  const int h = m + w - 1, J = n - h - 1;
  const int tend = J >= 1 ? J + w - 1 : 0;
  const std::vector<Run> want = J >= 1 ? brute(key, J, w) : std::vector<Run>();
  ++g_cases;
  g_runs += (long)want.size();
  // by the definition
  uint32_t P[N] = {};
  for (int t = w; t <= tend; ++t) {
    const int pos = window_min(key, t, w);
    P[(pos + m) >> 5] |= 1u << ((pos + m) & 31);
  }
  auto key_at = [&](int p) { return key[p]; };
  if (mg_runs::count<N>(P) != want.size()) return fail("run count", n, m, w);
  for (uint32_t i = 0; i <= want.size(); ++i) {
    Run r{};
    const bool ok = mg_runs::decode<N>(P, J, m, w, i, key_at, r.p, r.lo, r.hi);
    if (ok != (i < want.size())) return fail("decode: which runs exist", n, m, w);
    if (ok && !(r == want[i])) return fail("decode: run " + std::to_string(i), n, m, w);
  }
  if (w > 32) return 0;
  // the way the kernel records them: word k's steps are those with (t + m) / 32 = k
  uint32_t Pk[N] = {};
  uint32_t last_mn = 0;
  const int tmax = std::min(tend + tmax_extra, 32 * (N + 1) - 1 - m);
  const int tall = tend ? std::max(w, tend - tall_back) : 0;  // (a shorter neighbour ends the unguarded phase early)
  for (int k = 0; k <= N; ++k) {
    uint32_t spare_lo = 0, spare_hi = 0;
    uint32_t& plo = (k >= 1 && k - 1 < N) ? Pk[k - 1] : spare_lo;
    uint32_t& phi = k < N ? Pk[k] : spare_hi;
    const uint32_t cadd = (uint32_t)(m + 32 - 32 * k);
    const int t0 = std::max(1, 32 * k - m), t1 = std::min(tmax, 32 * k + 31 - m);
    for (int t = t0; t <= t1; ++t) {
      if (t < w) continue;
      // a lane without windows computes on whatever its slot holds
      const uint32_t mn = t <= tend ? key[window_min(key, t, w)] : (uint32_t)(t * 2654435761u);
      if (t == w || t <= tall)
        last_mn = mn;  // step_first's window 1 and step_all: unguarded
      else
        last_mn = t <= tend ? mn : last_mn;
      mg_runs::mark(plo, phi, last_mn + cadd);
    }
  }
  mg_runs::clip<N>(Pk, (int)(last_mn & 1023u) + m, tend > 0);
  for (int k = 0; k < N; ++k)
    if (Pk[k] != P[k]) return fail("the kernel's recording differs from the definition", n, m, w);
  const uint32_t cnt = mg_runs::count<N>(Pk);
  int xb = 0, jl = 1;
  for (int e = 0; e < 2; ++e) mg_runs::shift<N>(Pk, xb, mg_runs::NoCarry());
  // two trips more than the read has runs, as a lane of a wavefront with longer lists takes
  int pc = mg_runs::pop<N, 0>(Pk, xb, mg_runs::NoCarry()) - m;
  for (uint32_t i = 0; i < cnt + 2; ++i) {
    const int pn = mg_runs::pop<N, 0>(Pk, xb, mg_runs::NoCarry()) - m;
    const bool last = i + 1 >= cnt;
    if (i < cnt) {
      // (the kernel computes the successor's key from whatever bits the pop returned; only a real successor's counts)
      const Run r{pc, jl, mg_runs::run_end(pc, key[pc], pn, last ? 0u : key[pn], last, J, w)};
      if (!(r == want[i])) return fail("emission: run " + std::to_string(i), n, m, w);
      jl = r.hi + 1;
    }
    pc = pn;
  }
  return 0;
}

enum Kind { RANDOM, EQUAL, UP, DOWN, FEW };

std::vector<uint32_t> keys(std::mt19937_64& rng, int count, Kind kind) {
  std::vector<uint32_t> k(count);
  for (int t = 0; t < count; ++t) {
    const uint32_t v = kind == RANDOM ? (uint32_t)(rng() & 0x3FFFFF)
                       : kind == EQUAL ? 77u
                       : kind == UP    ? (uint32_t)t
                       : kind == DOWN  ? (uint32_t)(5000 - t)
                                       : (uint32_t)(rng() % 3);  // many ties
    k[t] = (v << 10) | (uint32_t)t;                              // order key | position: leftmost on ties
  }
  return k;
}

template <int N>
int sweep(std::mt19937_64& rng) {
  const int edges[] = {1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 191, 192, 223, 224, 255, 256};
  const int ws[] = {1, 2, 19, 31, 32, 33, 65, 70};
  const int ms[] = {1, 15, 32};
  for (int w : ws)
    for (int m : ms) {
      const int h = m + w - 1;
      std::vector<int> ns;
      for (int e : edges) {
        ns.push_back(e + m);      // n - m on the edge
        ns.push_back(e + h + 1);  // J on the edge
      }
      ns.push_back(h + 2);  // n = l + 1: one window
      ns.push_back(32 * N);
      ns.push_back(32 * N - 1);
      for (int n : ns) {
        if (n > 32 * N || n < h + 1 || n - m + 1 < 1) continue;
        for (Kind kind : {RANDOM, EQUAL, UP, DOWN, FEW})
          for (int extra : {0, 300}) {
            if (check<N>(keys(rng, n - m + 1, kind), n, m, w, extra, extra ? (int)(rng() % 70) : 0)) return 1;
            if (kind != RANDOM && kind != FEW) break;
          }
      }
    }
  return 0;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20240611);
  if (sweep<1>(rng) || sweep<2>(rng) || sweep<3>(rng) || sweep<5>(rng) || sweep<8>(rng)) return 1;
  // all keys equal: every window is its own run, the maximum count
  {
    const int n = 256, m = 15, w = 19, J = n - (m + w - 1) - 1;
    const std::vector<uint32_t> k = keys(rng, n - m + 1, EQUAL);
    if ((int)brute(k, J, w).size() != J) return fail("equal keys give J runs", n, m, w);
  }
  std::printf("mg_runs_check: ok (%ld reads, %ld runs)\n", g_cases, g_runs);
  return 0;
}
