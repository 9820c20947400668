// Host check of the rank order the geometry kernels scatter by (diffusion_pullback_amd/csrc/rank.h): for every value set and every k, the scatter
// order[rank_desc(v, k, t)] = t into a poisoned array must leave a permutation of 0 .. k-1 that lists the values descending, NaN first, ties by index;
// and max_nan must keep a NaN where fmax drops it.  Built with -fsanitize=address,undefined by tests/test_rank_order_host.py: an index outside
// [0, k) is a sanitizer report as well as a failed check.  Exit status 0 and a last line "rank-order ok <cases>" mean every check held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "rank.h"

namespace {

constexpr int POISON = -12345;
const double NaN = std::numeric_limits<double>::quiet_NaN();
const double INF = std::numeric_limits<double>::infinity();
int failures = 0, cases = 0;

void fail(const std::string& set, int k, const char* what, int at) {
  std::printf("FAIL %s k=%d: %s at %d\n", set.c_str(), k, what, at);
  ++failures;
}

// the order the scatter must produce, stated independently: a stable insertion sort by (NaN first, then descending value)
std::vector<int> expected_order(const std::vector<double>& v) {
  const int k = (int)v.size();
  std::vector<int> o;
  for (int t = 0; t < k; ++t) {
    size_t at = o.size();
    while (at > 0) {
      const double prev = v[o[at - 1]], mine = v[t];
      const bool prev_stays = std::isnan(prev) || (!std::isnan(mine) && prev >= mine);      // equal values: the earlier index stays in front
      if (prev_stays) break;
      --at;
    }
    o.insert(o.begin() + at, t);
  }
  return o;
}

void check(const std::string& set, const std::vector<double>& v) {
  const int k = (int)v.size();
  ++cases;
  std::vector<int> order(k, POISON), seen(k, 0);       // heap arrays of exactly k ints: ASan sees one slot past either end
  for (int t = 0; t < k; ++t) {
    const int r = dpb::rank_desc(v.data(), k, t);
    if (r < 0 || r >= k) { fail(set, k, "rank outside [0, k)", t); return; }
    order[r] = t;
  }
  for (int i = 0; i < k; ++i) {
    if (order[i] == POISON) { fail(set, k, "slot left unwritten", i); return; }
    if (order[i] < 0 || order[i] >= k || seen[order[i]]++) { fail(set, k, "not a permutation", i); return; }
  }
  const std::vector<int> want = expected_order(v);
  for (int i = 0; i < k; ++i)
    if (order[i] != want[i]) { fail(set, k, "order differs from NaN first, descending, ties by index", i); return; }
  for (int i = 0; i + 1 < k; ++i) {                    // the same property read off the values
    const double a = v[order[i]], b = v[order[i + 1]];
    if (std::isnan(b) && !std::isnan(a)) { fail(set, k, "a NaN behind a number", i); return; }
    if (!std::isnan(a) && !std::isnan(b) && a < b) { fail(set, k, "ascending pair", i); return; }
    const bool tie = (std::isnan(a) && std::isnan(b)) || a == b;
    if (tie && order[i] > order[i + 1]) { fail(set, k, "tie not in index order", i); return; }
  }
}

// the plain comparison the kernels used to rank by: kept here to show what the check is for (every NaN gets rank 0)
int rank_plain(const double* v, int k, int t) {
  int rank = 0;
  for (int e = 0; e < k; ++e) rank += (v[e] > v[t] || (v[e] == v[t] && e < t)) ? 1 : 0;
  return rank;
}

}  // namespace

int main() {
  const int ks[] = {1, 2, 5, 6, 16, 17, 33, 64, 65, 97, 128};
  for (int k : ks) {
    std::vector<double> base(k);
    for (int i = 0; i < k; ++i) base[i] = std::ldexp(1.0, -(i % 7)) * (1 + (i * 37) % 11);      // distinct-ish finite values, not sorted
    check("all-nan", std::vector<double>(k, NaN));
    for (int pos : {0, k / 2, k - 1}) {
      std::vector<double> v = base;
      v[pos] = NaN;
      check("one-nan@" + std::to_string(pos), v);
    }
    {
      const double mix[] = {NaN, INF, -INF, 0.0, -0.0, 1.5, NaN, -2.0};
      std::vector<double> v(k);
      for (int i = 0; i < k; ++i) v[i] = mix[(i * 5 + 3) % 8];
      check("nan-inf-zero-mix", v);
      for (int i = 0; i < k; ++i) v[i] = mix[i % 5];   // NaN, +inf, -inf, +0, -0 only
      check("nan-inf-zero-only", v);
    }
    check("all-equal", std::vector<double>(k, 2.0));
    check("all-zero", std::vector<double>(k, 0.0));
    {
      // the tie pattern of tests/_orth_ref.py (TIE_SEEDS): squared sigma from {4, 2, 1} in tie groups, at k = 5 the shuffle (2, 1, 4, 2, 4)
      const double five[] = {4.0, 1.0, 16.0, 4.0, 16.0};
      std::vector<double> v(k);
      for (int i = 0; i < k; ++i) v[i] = k == 5 ? five[i] : five[(i * 3 + i / 5) % 5];
      check("ties", v);
      if (k > 2) { v[k / 2] = NaN; check("ties+nan", v); }
    }
    check("finite", base);
  }
  {
    // the defect the total order closes: under the plain comparison an all-NaN input of k > 1 leaves slots of `order` unwritten
    const int k = 6;
    std::vector<double> v(k, NaN);
    std::vector<int> order(k, POISON);
    for (int t = 0; t < k; ++t) order[rank_plain(v.data(), k, t)] = t;
    int unwritten = 0;
    for (int i = 0; i < k; ++i) unwritten += order[i] == POISON;
    if (unwritten != k - 1) { std::printf("FAIL the plain comparison was expected to leave %d slots unwritten, left %d\n", k - 1, unwritten); ++failures; }
  }
  {
    const float n = std::numeric_limits<float>::quiet_NaN();
    bool ok = std::isnan(dpb::max_nan(0.f, n)) && std::isnan(dpb::max_nan(n, 0.f)) && std::isnan(dpb::max_nan(n, n)) && std::isnan(dpb::max_nan(NaN, 1.0)) &&
              std::isnan(dpb::max_nan(1.0, NaN)) && dpb::max_nan(1.f, 2.f) == 2.f && dpb::max_nan(2.f, 1.f) == 2.f && dpb::max_nan(-1.0, 0.0) == 0.0 &&
              dpb::max_nan(0.f, std::numeric_limits<float>::infinity()) == std::numeric_limits<float>::infinity() && !std::isnan(std::fmax(0.f, n));
    if (!ok) { std::printf("FAIL max_nan\n"); ++failures; }
  }
  if (failures) { std::printf("rank-order FAILED %d of %d\n", failures, cases); return 1; }
  std::printf("rank-order ok %d\n", cases);
  return 0;
}
