// Mutation harness for the host stage of gb_verify_compressed_batch (csrc/verify_batch_host.inc over csrc/compress_host.inc's parser
// and csrc/verify_compressed.hpp's sibling count), linked against the HOST-ONLY build of the library compiled with
// -fsanitize=address,undefined (tests/sanitize/build_compressed_batch.py).  CPU only: the context is NULL, so the call runs its host
// stage and nothing else - a proof the host decides gets its verdict, a proof that would go to a device is answered GB_ERR_INVALID
// with check 0, and the call itself returns GB_ERR_INVALID for the null context.  Includes nothing but the public header.
//
//   fuzz_compressed_batch <case-file> <iterations> <seed>
// case file: as for fuzz_host_parsers.cpp (tests/test_sanitized_parsers.py writes it).
// Every proof whose verdict the host stage gives must carry what gb_verify_compressed says of it (status and text); every proof left to
// the device must be one gb_verify_compressed does not refuse as malformed before the query rounds.  Anything else, or a sanitizer
// report, fails the run.  Prints one summary line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "goldibear_gpu.h"

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// truncated, bit-flipped, spliced and extended; `other` lends the runs that are spliced in
static std::vector<uint8_t> mutate(const std::vector<uint8_t>& src, const std::vector<uint8_t>& other) {
    std::vector<uint8_t> m = src;
    switch (rnd() % 8) {
        case 0:
            m.resize(rnd() % (m.size() + 1));
            break;
        case 1:
            if (!m.empty()) m[rnd() % m.size()] ^= (uint8_t)(1u << (rnd() % 8));
            break;
        case 2:  // a byte: the path length bytes among them
            if (!m.empty()) m[rnd() % m.size()] = (uint8_t)rnd();
            break;
        case 3: {  // a length byte moved by one: the nearest byte below 32 behind a random place
            if (m.empty()) break;
            size_t at = rnd() % m.size();
            while (at < m.size() && m[at] >= 32) at++;
            if (at < m.size()) m[at] = (uint8_t)(m[at] + (rnd() & 1 ? 1 : -1));
            break;
        }
        case 4: {
            const size_t n = 1 + rnd() % 64;
            for (size_t i = 0; i < n; i++) m.push_back((uint8_t)rnd());
            break;
        }
        case 5: {  // cut a run out
            if (m.size() < 2) break;
            const size_t a = rnd() % m.size(), n = 1 + rnd() % std::min<size_t>(64, m.size() - a);
            m.erase(m.begin() + a, m.begin() + a + n);
            break;
        }
        case 6: {  // splice a run of another proof's bytes in, in place or inserted
            if (m.empty() || other.empty()) break;
            const size_t a = rnd() % m.size(), b = rnd() % other.size(), n = 1 + rnd() % std::min<size_t>(96, other.size() - b);
            if (rnd() & 1) m.insert(m.begin() + a, other.begin() + b, other.begin() + b + n);
            else std::memcpy(&m[a], &other[b], std::min(n, m.size() - a));
            break;
        }
        default: {  // a whole hash appended behind a random place (a surplus sibling where the place is a path's end)
            const size_t a = m.empty() ? 0 : rnd() % m.size();
            m.insert(m.begin() + a, 32, (uint8_t)1);
            break;
        }
    }
    return m;
}

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s case-file iterations seed\n", argv[0]);
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> file;
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + got);
    std::fclose(f);
    const long iterations = std::atol(argv[2]);
    rng_state = std::strtoull(argv[3], nullptr, 0);
    size_t off = 0;
    auto take = [&](void* dst, size_t n) {
        if (off + n > file.size()) { std::fprintf(stderr, "short case file\n"); std::exit(2); }
        std::memcpy(dst, &file[off], n);
        off += n;
    };
    gb_circuit_config cfg;
    take(&cfg, sizeof cfg);
    uint32_t num_gates;
    take(&num_gates, 4);
    std::vector<gb_gate> gates(num_gates);
    take(gates.data(), num_gates * sizeof(gb_gate));
    const size_t es = cfg.field == GB_GOLDILOCKS ? 8 : 4, H = cfg.field == GB_GOLDILOCKS ? 4 : 8;
    std::vector<uint8_t> k_is(cfg.num_routed_wires * es), cap((H << cfg.cap_height) * es), digest(H * es);
    take(k_is.data(), k_is.size());
    take(cap.data(), cap.size());
    take(digest.data(), digest.size());
    uint64_t proof_len;
    take(&proof_len, 8);
    std::vector<uint8_t> proof(proof_len);
    take(proof.data(), proof_len);

    gb_circuit* c = nullptr;
    gb_status s = gb_verifier_create(nullptr, &cfg, gates.data(), num_gates, k_is.data(), cap.data(), digest.data(), &c);
    if (s != GB_OK) { std::fprintf(stderr, "gb_verifier_create: %d %s\n", s, gb_last_error(nullptr)); return 1; }
    std::vector<uint8_t> out(2 * proof.size() + (1 << 16));
    size_t n = 0;
    s = gb_proof_compress(c, proof.data(), proof.size(), out.data(), out.size(), &n);
    if (s != GB_OK) { std::fprintf(stderr, "compress: %d %s\n", s, gb_last_error(nullptr)); return 1; }
    const std::vector<uint8_t> compressed(out.begin(), out.begin() + n);

    // batches of four: mutants, and every few rounds the honest proof and an empty one among them
    long host_decided = 0, left_to_device = 0, statuses[3] = {};
    for (long it = 0; it < iterations; it++) {
        std::vector<std::vector<uint8_t>> batch;
        for (int k = 0; k < 4; k++) batch.push_back(mutate(compressed, k & 1 ? proof : compressed));
        if (it % 5 == 0) batch[1] = compressed;
        if (it % 7 == 0) batch[2].clear();
        const void* ptrs[4];
        size_t lens[4];
        static const uint8_t nothing = 0;
        for (int k = 0; k < 4; k++) { ptrs[k] = batch[k].empty() ? &nothing : batch[k].data(); lens[k] = batch[k].size(); }
        gb_verify_result res[4];
        std::memset(res, 0xAB, sizeof res);
        s = gb_verify_compressed_batch(nullptr, c, ptrs, lens, 4, 0, res);
        if (s != GB_ERR_INVALID || !std::strstr(gb_last_error(nullptr), "null ctx")) {
            std::fprintf(stderr, "the call without a context returned %d (%s)\n", s, gb_last_error(nullptr));
            return 1;
        }
        for (int k = 0; k < 4; k++) {
            const gb_status want = gb_verify_compressed(c, ptrs[k], lens[k]);
            const std::string text = want == GB_OK ? "" : gb_last_error(nullptr);
            if (want != GB_OK && want != GB_ERR_INVALID && want != GB_ERR_VERIFY) {
                std::fprintf(stderr, "gb_verify_compressed returned %d (%s) on a mutated input\n", want, text.c_str());
                return 1;
            }
            statuses[want == GB_OK ? 0 : want == GB_ERR_INVALID ? 1 : 2]++;
            const gb_verify_result& r = res[k];
            if (r.status == GB_ERR_INVALID && r.check == GB_VCHECK_NONE) {   // left to the device: the parser, the indices and the
                left_to_device++;                                            // sibling count had nothing to say
                const char* host_only[] = {"truncated", "non-canonical", "trailing", "public inputs", "query indices", "missing a sibling"};
                for (const char* h : host_only)
                    if (want != GB_OK && text.find(h) != std::string::npos) {
                        std::fprintf(stderr, "iteration %ld: a proof gb_verify_compressed refuses with '%s' was left to the device\n", it, text.c_str());
                        return 1;
                    }
                continue;
            }
            host_decided++;
            if ((gb_status)r.status != want || text != gb_verify_check_text(r.check)) {
                std::fprintf(stderr, "iteration %ld: host stage says %u '%s', gb_verify_compressed %d '%s'\n", it, r.status,
                             gb_verify_check_text(r.check), want, text.c_str());
                return 1;
            }
        }
    }
    gb_circuit_free(c);
    std::printf("fuzz ok: %ld iterations; host decided %ld, left to the device %ld; gb_verify_compressed ok/invalid/verify = %ld/%ld/%ld\n",
                iterations, host_decided, left_to_device, statuses[0], statuses[1], statuses[2]);
    return 0;
}
