// posterior_gather_check.cpp -- the shard gather of fst_posterior_lhs_batch on the CPU
// (csrc/posterior_gather.hpp: host code with no device call of its own), as a stand-alone program
// for a sanitizer build:
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined posterior_gather_check.cpp -o check && ./check
// Random batches (items of zero states, states of zero arcs, a first state offset above zero) are
// cut into 1 to 9 contiguous shards; every shard's arrays are made as run_posterior_shard leaves
// them, exactly as long as the shard's ranges, and gathered with memcpy into result arrays of
// exactly the caller's extents.  Every entry must hold the value of its own global index, the
// entries in front of the first item +inf, and the sanitizer must see no access outside any
// array.  Prints "posterior_gather_check: ok".
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../csrc/posterior_gather.hpp"

using namespace fstamd::host;

static int fail(const char* what, unsigned seed) {
  std::printf("posterior_gather_check: FAILED (%s, seed %u)\n", what, seed);
  return 1;
}

int main() {
  for (unsigned seed = 0; seed < 400; ++seed) {
    std::mt19937 rng(seed);
    const uint32_t num = 1 + rng() % 40;
    std::vector<uint64_t> so(num + 1);
    so[0] = rng() % 3 ? 0 : rng() % 5;  // (state_offsets[0] need not be 0)
    for (uint32_t i = 0; i < num; ++i) so[i + 1] = so[i] + (rng() % 4 ? rng() % 7 : 0);
    const uint64_t states = so[num];
    std::vector<uint64_t> ao(states + 1);
    ao[0] = 0;
    for (uint64_t s = 0; s < states; ++s) ao[s + 1] = ao[s] + (rng() % 3 ? rng() % 5 : 0);
    const uint64_t arcs = ao[states];
    // the result, exactly the caller's extents (no slack: an overrun is the sanitizer's to see)
    std::vector<int32_t> status(num, -1);
    std::vector<double> total(num, -1.0), alpha(states, -1.0), beta(states, -1.0),
        cost(arcs, -1.0);
    posterior_fill_front(so.data(), ao.data(), num, alpha.data(), beta.data(), cost.data());
    // the shard plan: contiguous item ranges, none empty
    uint32_t nsh = 1 + rng() % 9;
    if (nsh > num) nsh = num;
    std::vector<uint32_t> cut{0};
    for (uint32_t j = 1; j < nsh; ++j) {
      const uint32_t lo = cut.back() + 1, hi = num - (nsh - j);
      cut.push_back(lo + rng() % (hi - lo + 1));
    }
    cut.push_back(num);
    const auto copy = [](void* dst, const void* src, uint64_t bytes) {
      if (bytes) std::memcpy(dst, src, bytes);
      return true;
    };
    for (uint32_t j = 0; j < nsh; ++j) {
      const uint32_t s0 = cut[j], s1 = cut[j + 1];
      const PosteriorRanges r = posterior_shard_ranges(so.data(), ao.data(), s0, s1);
      if (r.sb + r.ns > states || r.ab + r.na > arcs) return fail("ranges", seed);
      std::vector<int32_t> st(s1 - s0);
      std::vector<double> tot(s1 - s0), vals(2 * r.ns + r.na);
      for (uint32_t i = s0; i < s1; ++i) {
        st[i - s0] = (int32_t)i;
        tot[i - s0] = 0.5 + i;
      }
      for (uint64_t s = 0; s < r.ns; ++s) {
        vals[s] = 1e6 + (double)(r.sb + s);
        vals[r.ns + s] = 2e6 + (double)(r.sb + s);
      }
      for (uint64_t a = 0; a < r.na; ++a) vals[2 * r.ns + a] = 3e6 + (double)(r.ab + a);
      if (!posterior_gather_shard(r, s0, s1, st.data(), tot.data(), vals.data(), status.data(),
                                  total.data(), alpha.data(), beta.data(), cost.data(), copy))
        return fail("copy", seed);
    }
    for (uint32_t i = 0; i < num; ++i)
      if (status[i] != (int32_t)i || total[i] != 0.5 + i) return fail("per-item arrays", seed);
    for (uint64_t s = 0; s < states; ++s) {
      const bool front = s < so[0];
      if (alpha[s] != (front ? HUGE_VAL : 1e6 + (double)s)) return fail("alpha", seed);
      if (beta[s] != (front ? HUGE_VAL : 2e6 + (double)s)) return fail("beta", seed);
    }
    for (uint64_t a = 0; a < arcs; ++a)
      if (cost[a] != (a < ao[so[0]] ? HUGE_VAL : 3e6 + (double)a)) return fail("arc_cost", seed);
  }
  std::printf("posterior_gather_check: ok\n");
  return 0;
}
