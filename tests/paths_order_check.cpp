// CPU checker of the rtx_trace_paths_keyed rules in
// raytrace-we-gpu_amd/csrc/rtx_paths.h (tests/test_paths_keyed_host.py): the
// argument rule and its order, the default probe, the two-phase rule, the cost
// bucket, and the three sort passes (k_paths_cost_keys, k_cast_prefix,
// k_cast_scatter) replayed workgroup by workgroup on host arrays of exactly
// the sizes the entry point allocates, so that an index past one is a
// sanitizer report. Prints one JSON line. Compiled plain and under ASan +
// UBSan.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "../raytrace-we-gpu_amd/csrc/rtx_paths.h"

namespace {

constexpr uint32_t kBuckets = 65536u;  // kCastBuckets (rtx_cast.h)
constexpr uint32_t kChunk = 2048u;     // kCastChunk (rtx_kernels.hip): records per workgroup
constexpr uint32_t kBlock = 256u;

uint32_t lcg(uint32_t &s) {
    s = s * 1664525u + 1013904223u;
    return s;
}

// The rule written out again, independently of the header's order of tests:
// the first failing one in the order include/rtx.h lists them.
int want_args(bool q, bool r, uint32_t n, uint32_t samples, uint32_t flags, bool keys, uint32_t probe) {
    if (n > 0 && !q) return 1;
    if (n > 0 && !r) return 2;
    if (samples == 0) return 3;
    if (flags != 0 && flags != 1 && flags != 2 && flags != 3) return 4;
    if (keys && probe != 0) return 5;
    return 0;
}

uint32_t ckey(uint32_t key) { return key < 65535u ? key : 65535u; }

// launch_paths_cost_order on host memory: src of exactly n words, counts of
// kBuckets, keys and perm of n. Returns the number of rule violations.
unsigned long long play(const std::vector<uint32_t> &src) {
    unsigned long long bad = 0;
    const uint32_t n = (uint32_t)src.size();
    std::vector<uint32_t> counts(kBuckets, 0u), keys(n, 0xffffffffu), perm(n, 0xffffffffu), written(n, 0u);
    const uint32_t blocks = (n + kChunk - 1u) / kChunk;
    // k_paths_cost_keys: a workgroup's table of the keys it meets, one global add per distinct key
    for (uint32_t b = 0; b < blocks; ++b) {
        std::map<uint32_t, uint32_t> table;
        for (uint32_t k = 0; k < kChunk / kBlock; ++k)
            for (uint32_t t = 0; t < kBlock; ++t) {
                const uint64_t i = (uint64_t)b * kChunk + k * kBlock + t;
                if (i >= n) continue;
                const uint32_t key = rtx::paths_cost_bucket(src.at(i));
                bad += key >= kBuckets;
                keys.at(i) = key;
                ++table[key];
            }
        for (const auto &e : table) counts.at(e.first) += e.second;
    }
    // k_cast_prefix: counts[b] -> the records in buckets below b
    uint32_t pre = 0;
    for (uint32_t b = 0; b < kBuckets; ++b) {
        const uint32_t c = counts[b];
        counts[b] = pre;
        pre += c;
    }
    bad += pre != n;
    // k_cast_scatter: rank within the workgroup's records of the key, one reservation per workgroup and key
    for (uint32_t b = 0; b < blocks; ++b) {
        std::map<uint32_t, uint32_t> cnt, first;
        std::vector<uint32_t> rank(kChunk, 0u);
        for (uint32_t j = 0; j < kChunk; ++j) {
            const uint64_t i = (uint64_t)b * kChunk + j;
            if (i >= n) continue;
            rank[j] = cnt[std::min(keys.at(i), kBuckets - 1u)]++;
        }
        for (const auto &e : cnt) {
            first[e.first] = counts.at(e.first);
            counts.at(e.first) += e.second;
        }
        for (uint32_t j = 0; j < kChunk; ++j) {
            const uint64_t i = (uint64_t)b * kChunk + j;
            if (i >= n) continue;
            const uint32_t g = first[std::min(keys.at(i), kBuckets - 1u)] + rank[j];
            if (g < n) {
                perm.at(g) = (uint32_t)i;
                ++written.at(g);
            } else {
                ++bad;
            }
        }
    }
    std::vector<uint32_t> seen(n, 0u);
    for (uint32_t g = 0; g < n; ++g) {
        bad += written[g] != 1u;  // every slot once
        if (perm[g] >= n || seen[perm[g]]++) {
            ++bad;  // a permutation
            continue;
        }
        if (g != 0 && perm[g - 1] < n && ckey(src[perm[g - 1]]) < ckey(src[perm[g]])) ++bad;  // non-increasing
    }
    return bad;
}

}  // namespace

int main() {
    unsigned long long arg_checks = 0, arg_bad = 0;
    const uint32_t ns[] = {0u, 1u, 64u, 0xffffffffu}, ss[] = {0u, 1u, 6u, 0xffffffffu};
    const uint32_t fs[] = {0u, 1u, 2u, 3u, 4u, 7u, 0x80000000u, 0xffffffffu}, ps[] = {0u, 1u, 2u, 0xffffffffu};
    for (int q = 0; q < 2; ++q)
        for (int r = 0; r < 2; ++r)
            for (uint32_t n : ns)
                for (uint32_t s : ss)
                    for (uint32_t f : fs)
                        for (int k = 0; k < 2; ++k)
                            for (uint32_t p : ps) {
                                ++arg_checks;
                                arg_bad += (int)rtx::paths_keyed_args(q != 0, r != 0, n, s, f, k != 0, p) !=
                                           want_args(q != 0, r != 0, n, s, f, k != 0, p);
                            }
    arg_bad += rtx::kPathsKeyedArgOk != 0 || rtx::kPathsKeyedArgQueries != 1 || rtx::kPathsKeyedArgResults != 2 ||
               rtx::kPathsKeyedArgSamples != 3 || rtx::kPathsKeyedArgFlags != 4 || rtx::kPathsKeyedArgProbe != 5;
    // rtx_trace_paths' own rule is as it was: order 3 is refused there
    arg_bad += rtx::paths_args(true, true, 5u, 6u, 0u, 3u) != rtx::kPathsArgOrder || rtx::kPathsOrderMax != 2u ||
               rtx::kPathsOrderCost != 3u;

    unsigned long long rule_bad = 0;
    // the refine pre-pass's rule: 2 samples, 1 above 1,024 padded spheres
    rule_bad += rtx::paths_default_probe(0u) != 2u || rtx::paths_default_probe(1024u) != 2u ||
                rtx::paths_default_probe(1032u) != 1u || rtx::paths_default_probe(0xffffffffu) != 1u;
    // two phases only when something is left after the probe
    for (uint32_t p : {1u, 2u, 6u, 0xffffffffu}) {
        rule_bad += rtx::paths_two_phase(p - 1u, p) != false;
        rule_bad += rtx::paths_two_phase(p, p) != false;
        if (p != 0xffffffffu) rule_bad += rtx::paths_two_phase(p + 1u, p) != true;
    }
    // the bucket: 65535 - min(key, 65535)
    rule_bad += rtx::paths_cost_bucket(0u) != 65535u || rtx::paths_cost_bucket(1u) != 65534u ||
                rtx::paths_cost_bucket(65534u) != 1u || rtx::paths_cost_bucket(65535u) != 0u ||
                rtx::paths_cost_bucket(65536u) != 0u || rtx::paths_cost_bucket(0xffffffffu) != 0u;
    rule_bad += rtx::kPathsCostBuckets != kBuckets || rtx::kPathsKeyMax != 65535u;
    uint32_t s = 77u;
    for (int k = 0; k < 100000; ++k) rule_bad += rtx::paths_cost_bucket(lcg(s) >> (k % 24)) >= kBuckets;

    // the sort passes on arrays of exactly n words
    unsigned long long sorts = 0, sort_bad = 0, words = 0;
    const uint32_t sizes[] = {1u, 63u, 65u, 2047u, 2048u, 2049u, 4099u};
    for (uint32_t n : sizes) {
        std::vector<uint32_t> src(n);
        for (uint32_t fill : {0u, 7u, 65535u, 0xffffffffu}) {  // all equal
            std::fill(src.begin(), src.end(), fill);
            sort_bad += play(src), ++sorts;
        }
        for (uint32_t i = 0; i < n; ++i) src[i] = i;  // all distinct, ascending: the order is reversed
        sort_bad += play(src), ++sorts;
        for (uint32_t i = 0; i < n; ++i) src[i] = n - 1u - i;  // ... descending: kept
        sort_bad += play(src), ++sorts;
        for (uint32_t i = 0; i < n; ++i) src[i] = (lcg(s) >> 16) & 1u ? 12u : 3u;  // two values
        sort_bad += play(src), ++sorts;
        for (uint32_t i = 0; i < n; ++i) src[i] = 2u + (lcg(s) >> 27);  // a few dozen, as a probe leaves
        sort_bad += play(src), ++sorts;
        for (uint32_t i = 0; i < n; ++i) {  // arbitrary words of every magnitude
            const uint32_t shift = lcg(s) >> 27;
            src[i] = lcg(s) >> shift;
        }
        sort_bad += play(src), ++sorts;
        words += 9ull * n;
    }
    std::printf("{\"arg_checks\": %llu, \"arg_bad\": %llu, \"rule_bad\": %llu, \"sorts\": %llu, \"words\": %llu, "
                "\"sort_bad\": %llu, \"order_cost\": %u, \"buckets\": %u}\n",
                arg_checks, arg_bad, rule_bad, sorts, words, sort_bad, rtx::kPathsOrderCost, rtx::kPathsCostBuckets);
    return arg_bad == 0 && rule_bad == 0 && sort_bad == 0 ? 0 : 1;
}
