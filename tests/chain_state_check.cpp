// chain_state_check.cpp — the chain-state file of rtx_cli (rtx_app.cpp
// write_chain_state / read_chain_state) on synthetic states, no GPU:
//   chain_state_check DIR
// Writes states of 7x5, 1x1 and 64x3 pixels holding NaNs, denormals, -0 and
// infinities and reads them back with identical bits; then damages a file in
// every way read_chain_state must refuse. Prints one JSON line; exit 0 when
// every check held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/rtx_app.hpp"

static std::vector<unsigned char> slurp(const std::string &p) {
    std::vector<unsigned char> b;
    FILE *f = std::fopen(p.c_str(), "rb");
    if (!f) return b;
    unsigned char buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
    std::fclose(f);
    return b;
}
static bool spit(const std::string &p, const std::vector<unsigned char> &b, size_t n) {
    FILE *f = std::fopen(p.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(b.data(), 1, n, f) == n;
    return std::fclose(f) == 0 && ok;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const std::string dir = argv[1];
    int round_trips = 0, refusals = 0, failures = 0;
    std::string log;
    auto expect_refused = [&](const std::string &path, const rtx::ChainStateHeader &want, const char *word,
                              const char *what) {
        std::vector<float> st;
        uint32_t n = 0;
        std::string err;
        if (rtx::read_chain_state(path, want, st, n, err) || err.find(word) == std::string::npos) {
            ++failures;
            log += std::string(what) + " not refused as expected (" + err + "); ";
        } else {
            ++refusals;
        }
    };
    const uint32_t sizes[3][2] = {{7, 5}, {1, 1}, {64, 3}};
    for (const auto &wh : sizes) {
        rtx::ChainStateHeader h;
        h.width = wh[0];
        h.height = wh[1];
        h.samples = 1000u + wh[0];
        h.world_hash = 0x0123456789abcdefull ^ wh[0];
        h.frame_hash = 0xfedcba9876543210ull ^ wh[1];
        std::vector<uint32_t> bits(4 * (size_t)h.width * h.height);
        uint32_t x = 0x9e3779b9u * (h.width + 1);
        for (size_t i = 0; i < bits.size(); ++i) {
            x = x * 1664525u + 1013904223u;
            bits[i] = x;
        }
        const uint32_t special[] = {0x7fc00000u, 0xffc12345u, 0x7f800001u, 0x00000001u, 0x807fffffu,
                                    0x80000000u, 0x7f800000u, 0xff800000u, 0u};
        for (size_t i = 0; i < sizeof special / sizeof *special; ++i) bits[(i * 3) % bits.size()] = special[i];
        std::vector<float> state(bits.size());
        std::memcpy(state.data(), bits.data(), bits.size() * 4);
        const std::string path = dir + "/s" + std::to_string(h.width) + "x" + std::to_string(h.height) + ".bin";
        if (!rtx::write_chain_state(path, h, state.data())) {
            ++failures;
            log += "write failed; ";
            continue;
        }
        std::vector<float> back;
        uint32_t n = 0;
        std::string err;
        if (!rtx::read_chain_state(path, h, back, n, err) || n != h.samples || back.size() != state.size() ||
            std::memcmp(back.data(), bits.data(), bits.size() * 4) != 0) {
            ++failures;
            log += "round trip " + path + " (" + err + "); ";
        } else {
            ++round_trips;
        }
        const std::vector<unsigned char> file = slurp(path);
        if (file.size() != 40 + 16 * (size_t)h.width * h.height) {
            ++failures;
            log += "file length; ";
            continue;
        }
        const std::string bad = path + ".bad";
        // truncated: the payload's last byte missing; then only half a header
        spit(bad, file, file.size() - 1);
        expect_refused(bad, h, "truncated", "a truncated payload");
        spit(bad, file, 20);
        expect_refused(bad, h, "truncated", "a truncated header");
        // a flipped magic byte
        std::vector<unsigned char> m = file;
        m[3] ^= 0x20;
        spit(bad, m, m.size());
        expect_refused(bad, h, "magic", "a flipped magic byte");
        // another format version
        m = file;
        m[8] = 2;
        spit(bad, m, m.size());
        expect_refused(bad, h, "version", "another version");
        // the header's width disagrees with the payload length
        m = file;
        m[12] = (unsigned char)(m[12] + 1);
        spit(bad, m, m.size());
        rtx::ChainStateHeader wider = h;
        wider.width = h.width + 1;  // even a caller who expects the header's size
        expect_refused(bad, wider, "length", "a width that disagrees with the length");
        // ... and so do bytes after the payload
        m = file;
        m.push_back(0);
        spit(bad, m, m.size());
        expect_refused(bad, h, "does not match its length", "a byte after the payload");
        // the caller's size, world or frame differs
        rtx::ChainStateHeader o = h;
        o.height = h.height + 1;
        expect_refused(path, o, "size mismatch", "another size");
        o = h;
        o.world_hash ^= 1;
        expect_refused(path, o, "world mismatch", "another world");
        o = h;
        o.frame_hash ^= 1ull << 63;
        expect_refused(path, o, "frame mismatch", "another frame");
    }
    std::vector<float> st;
    uint32_t n = 0;
    std::string err;
    if (rtx::read_chain_state(dir + "/none.bin", rtx::ChainStateHeader(), st, n, err)) ++failures;
    // the hashes see every input
    float sph[8] = {0, 1, 2, 3, 4, 5, 6, 7}, mt[2] = {0, 1}, mv[8] = {1, 1, 1, 0, 2, 2, 2, 0};
    const uint64_t w0 = rtx::chain_world_hash(2, 50, sph, mt, mv);
    int hash_changes = 0;
    hash_changes += rtx::chain_world_hash(1, 50, sph, mt, mv) != w0;
    hash_changes += rtx::chain_world_hash(2, 49, sph, mt, mv) != w0;
    sph[7] = 7.5f;
    hash_changes += rtx::chain_world_hash(2, 50, sph, mt, mv) != w0;
    sph[7] = 7.0f;
    mt[1] = 2.0f;
    hash_changes += rtx::chain_world_hash(2, 50, sph, mt, mv) != w0;
    mt[1] = 1.0f;
    mv[3] = 0.5f;
    hash_changes += rtx::chain_world_hash(2, 50, sph, mt, mv) != w0;
    mv[3] = 0.0f;
    hash_changes += rtx::chain_world_hash(2, 50, sph, mt, mv) == w0;
    rtx_frame f{};
    const uint64_t f0 = rtx::chain_frame_hash(f);
    f.frame_index = 1;
    hash_changes += rtx::chain_frame_hash(f) != f0;
    f.frame_index = 0;
    f.lens_v[3] = 1.0f;  // the struct's last word
    hash_changes += rtx::chain_frame_hash(f) != f0;
    // FNV-1a 64 of eight zero bytes (count 0, depth 0, no arrays): a known value
    const bool fnv_ok = rtx::chain_world_hash(0, 0, nullptr, nullptr, nullptr) == 0xa8c7f832281a39c5ull;
    if (hash_changes != 8 || !fnv_ok) {
        ++failures;
        log += "hashes; ";
    }
    std::printf("{\"round_trips\": %d, \"refusals\": %d, \"hash_changes\": %d, \"fnv_ok\": %s, \"failures\": %d, "
                "\"log\": \"%s\"}\n",
                round_trips, refusals, hash_changes, fnv_ok ? "true" : "false", failures, log.c_str());
    return failures == 0 ? 0 : 1;
}
