// Mutation harness for the parser of constraint programs (csrc/prover_host.inc parse_programs / build_gate_set, reached through
// gb_verifier_create_programs) and the interpreter the verifier runs on what it accepted (csrc/gates.hpp run_program), linked
// against a HOST-ONLY build of the library compiled with -fsanitize=address,undefined (the recipe is in
// tests/test_sanitized_gate_programs.py).  CPU only: gb_verifier_create_programs touches no device.  Includes nothing but the
// public header.
//
//   fuzz_gate_programs <case-file> <iterations> <seed>
// case file (written by the test from the reference's regression fixture with its gates as programs):
//   gb_circuit_config | u32 num_gates | gb_gate[num_gates] | k_is[num_routed_wires] | cap[2^cap_height][H] | digest[H] |
//   u32 num_programs | u32 offsets[num_programs + 1] | u64 words[offsets[num_programs]] | u64 proof_len | proof bytes
// Mutations of the program table: truncation, bit flips in header / literal / instruction words, index rewrites, a corrupted
// offset table (offsets stay inside the buffer: they describe it), oversized headers, a gate pointing at another program.  The
// table is handed over in a heap block of exactly the size the offsets describe, so a read past it is a sanitizer report.
// Every call must answer GB_OK / GB_ERR_INVALID (create) and GB_OK / GB_ERR_INVALID / GB_ERR_VERIFY (verify).  One summary line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "goldibear_gpu.h"

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return n ? (uint32_t)(rnd() % n) : 0; }

struct Reader {
    std::vector<uint8_t> d;
    size_t pos = 0;
    void take(void* out, size_t n) {
        if (pos + n > d.size()) { std::fprintf(stderr, "case file too short\n"); std::exit(2); }
        std::memcpy(out, d.data() + pos, n);
        pos += n;
    }
};

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: fuzz_gate_programs <case> <iterations> <seed>\n"); return 2; }
    Reader r;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
        uint8_t buf[1 << 16];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) r.d.insert(r.d.end(), buf, buf + n);
        std::fclose(f);
    }
    const long iterations = std::atol(argv[2]);
    rng_state = std::strtoull(argv[3], nullptr, 0);

    gb_circuit_config cfg;
    r.take(&cfg, sizeof cfg);
    uint32_t num_gates;
    r.take(&num_gates, 4);
    std::vector<gb_gate> gates(num_gates);
    r.take(gates.data(), num_gates * sizeof(gb_gate));
    const size_t el = cfg.field == GB_GOLDILOCKS ? 8 : 4, H = cfg.field == GB_GOLDILOCKS ? 4 : 8;
    std::vector<uint8_t> k_is(cfg.num_routed_wires * el), cap((H << cfg.cap_height) * el), digest(H * el);
    r.take(k_is.data(), k_is.size());
    r.take(cap.data(), cap.size());
    r.take(digest.data(), digest.size());
    uint32_t num_programs;
    r.take(&num_programs, 4);
    std::vector<uint32_t> offsets(num_programs + 1);
    r.take(offsets.data(), offsets.size() * 4);
    std::vector<uint64_t> words(offsets.back());
    r.take(words.data(), words.size() * 8);
    uint64_t proof_len;
    r.take(&proof_len, 8);
    std::vector<uint8_t> proof(proof_len);
    r.take(proof.data(), proof.size());

    long created = 0, refused = 0, v_ok = 0, v_invalid = 0, v_verify = 0;
    auto run = [&](const std::vector<gb_gate>& g, const std::vector<uint64_t>& w, const std::vector<uint32_t>& off, uint32_t np, bool must_verify) {
        // exact-size heap copies: the sanitizer sees any read past what the offsets describe
        uint64_t* wp = (uint64_t*)std::malloc(w.size() * 8 + 1);
        uint32_t* op = (uint32_t*)std::malloc(off.size() * 4 + 1);
        std::memcpy(wp, w.data(), w.size() * 8);
        std::memcpy(op, off.data(), off.size() * 4);
        gb_circuit* c = nullptr;
        const gb_status s = gb_verifier_create_programs(nullptr, &cfg, g.data(), (uint32_t)g.size(), wp, op, np, k_is.data(), cap.data(),
                                                        digest.data(), &c);
        std::free(wp);   // the library keeps its own copy
        std::free(op);
        if (s != GB_OK && s != GB_ERR_INVALID) { std::fprintf(stderr, "create answered %d: %s\n", s, gb_last_error(nullptr)); std::exit(1); }
        if (s != GB_OK) {
            if (c || must_verify) { std::fprintf(stderr, "create failed (%s) %s\n", gb_last_error(nullptr), c ? "and left an object" : "on the unmutated table"); std::exit(1); }
            refused++;
            return;
        }
        created++;
        const gb_status v = gb_verify(c, proof.data(), proof.size());
        if (v == GB_OK) v_ok++; else if (v == GB_ERR_INVALID) v_invalid++; else if (v == GB_ERR_VERIFY) v_verify++;
        else { std::fprintf(stderr, "verify answered %d: %s\n", v, gb_last_error(nullptr)); std::exit(1); }
        if (must_verify && v != GB_OK) { std::fprintf(stderr, "the unmutated programs do not verify: %s\n", gb_last_error(nullptr)); std::exit(1); }
        gb_circuit_free(c);
    };
    run(gates, words, offsets, num_programs, true);

    for (long it = 0; it < iterations; it++) {
        std::vector<gb_gate> g = gates;
        std::vector<uint64_t> w = words;
        std::vector<uint32_t> off = offsets;
        uint32_t np = num_programs;
        const uint32_t victim = below(num_programs), lo = offsets[victim], hi = offsets[victim + 1];
        switch (below(8)) {
            case 0: {   // truncation: the table ends inside (or right at the start of) a program
                const uint32_t cut = lo + below(hi - lo);
                w.resize(cut);
                np = victim + 1;
                off.resize(np + 1);
                off[np] = cut;
                break;
            }
            case 1:     // a bit flip anywhere in the victim
                w[lo + below(hi - lo)] ^= 1ull << below(64);
                break;
            case 2: {   // an operand or destination index rewritten
                const uint32_t nlit = (uint32_t)(w[lo + 2] >> 32), nins = (uint32_t)w[lo + 3];
                if (nins == 0 || lo + 4 + nlit + nins > hi) break;
                uint64_t& ins = w[lo + 4 + nlit + below(nins)];
                const uint32_t shift = below(3) == 0 ? 2 : below(2) ? 10 : 34, width = shift == 2 ? 6 : 22;
                ins = (ins & ~(((1ull << width) - 1) << shift)) | ((rnd() & ((1ull << width) - 1) & (below(2) ? 0xFFull : ~0ull)) << shift);
                break;
            }
            case 3:     // an operand's space rewritten
            {
                const uint32_t nlit = (uint32_t)(w[lo + 2] >> 32), nins = (uint32_t)w[lo + 3];
                if (nins == 0 || lo + 4 + nlit + nins > hi) break;
                uint64_t& ins = w[lo + 4 + nlit + below(nins)];
                const uint32_t shift = below(2) ? 8 : 32;
                ins = (ins & ~(3ull << shift)) | ((uint64_t)below(4) << shift);
                break;
            }
            case 4:     // the offset table: one entry anywhere inside the buffer
                off[below(num_programs + 1)] = below((uint32_t)w.size() + 1);
                break;
            case 5: {   // oversized or random header fields
                uint64_t& h = w[lo + below(4)];
                const uint64_t big[] = {0xFFFFFFFFull, 0xFFFFFFFF00000000ull, ~0ull, 4097, 33ull, 257ull << 32, 1025, 0x80000000ull, 0};
                h = below(2) ? big[below(9)] : (h & 0xFFFFFFFF00000000ull) | (uint32_t)(rnd() >> below(32));
                break;
            }
            case 6: {   // a literal out of the field, or any other word
                const uint32_t nlit = (uint32_t)(w[lo + 2] >> 32);
                if (nlit && lo + 4 + nlit <= hi) w[lo + 4 + below(nlit)] = below(2) ? ~0ull - below(1u << 20) : rnd();
                break;
            }
            default:    // a gate that names another program, or none
                for (auto& x : g)
                    if (x.kind == GB_GATE_PROGRAM && below(3) == 0) x.param = below(2) ? below(num_programs + 2) : (uint32_t)rnd();
                break;
        }
        run(g, w, off, np, false);
    }
    std::printf("fuzz ok: %ld mutations; create ok/invalid = %ld/%ld; verify ok/invalid/verify = %ld/%ld/%ld\n", iterations, created - 1, refused,
                v_ok - 1, v_invalid, v_verify);
    return 0;
}
