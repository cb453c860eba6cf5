// Mutation harness for the host stage of gb_fri_verify_batch (csrc/verify_batch_host.inc over csrc/verifier_host.inc's FriProof parser),
// linked against the HOST-ONLY build of the library compiled with -fsanitize=address,undefined
// (tests/sanitize/build_fri_verify_batch.py).  CPU only: the context is NULL, so the call runs its host stage and nothing else - an
// item the host decides gets its verdict, an item that would go to a device is answered GB_ERR_INVALID with check 0, and the call
// itself returns GB_ERR_INVALID for the null context.  Includes nothing but the public header.
//
//   fuzz_fri_verify_batch <case-file> <iterations> <seed>
// case file (tests/fri_batch_helpers.py write_case): u32 field, degree_bits, rate_bits, cap_height, hiding, num_oracles, num_batches,
// num_layers, proof_of_work_bits, num_query_rounds; u32 oracle_num_polys[], oracle_blinding[], batch_sizes[], polynomials[][2],
// reduction_arity_bits[]; one item: gb_challenger_state, points, openings, initial caps, u64 length, FriProof bytes.
// Every item whose verdict the host stage gives must carry what gb_fri_verify says of it (status and text); every item left to the
// device must have the shape's length and be one gb_fri_verify does not refuse in front of the query rounds' hashes.  Anything else,
// or a sanitizer report, fails the run.  Prints one summary line.
#include <algorithm>
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

// where the path-length bytes of the case's own (regular) proof stand, and how many bytes one sibling hash takes: walked once from
// the shape (main)
static std::vector<size_t> length_bytes;
static size_t hash_bytes;

// truncated, bit-flipped, spliced, extended; a true path-length byte moved by one, alone, with its path shortened or lengthened to
// match, or paired with another one moved the other way so that the proof keeps the shape's total length
static std::vector<uint8_t> mutate(const std::vector<uint8_t>& src) {
    std::vector<uint8_t> m = src;
    switch (rnd() % 11) {
        case 8: {   // a length byte alone: everything behind it is read at other offsets
            const size_t at = length_bytes[rnd() % length_bytes.size()];
            m[at] = (uint8_t)(m[at] + (rnd() & 1 ? 1 : -1));
            break;
        }
        case 9: {   // a path one sibling shorter or longer, its length byte with it: well-formed, of the wrong length
            const size_t at = length_bytes[rnd() % length_bytes.size()];
            const size_t end = at + 1 + (size_t)m[at] * hash_bytes;
            if (rnd() & 1) {
                m.insert(m.begin() + end, hash_bytes, (uint8_t)1);
                m[at]++;
            } else if (m[at]) {
                m.erase(m.begin() + (end - hash_bytes), m.begin() + end);
                m[at]--;
            }
            break;
        }
        case 10: {   // two length bytes, one up and one down: the shape's total length with irregular paths - what the regularity
                     // test exists for
            const size_t a = length_bytes[rnd() % length_bytes.size()], b = length_bytes[rnd() % length_bytes.size()];
            if (a == b || !m[b]) break;
            if (rnd() % 4 == 0) {   // the bytes alone: the words between them are read at other offsets
                m[a]++;
                m[b]--;
                break;
            }
            // well-formed: path a one sibling longer, path b one shorter (the later one first, so that the offsets hold)
            auto longer = [&m](size_t at) { m.insert(m.begin() + at + 1 + (size_t)m[at] * hash_bytes, hash_bytes, (uint8_t)1); m[at]++; };
            auto shorter = [&m](size_t at) {
                const size_t end = at + 1 + (size_t)m[at] * hash_bytes;
                m.erase(m.begin() + (end - hash_bytes), m.begin() + end);
                m[at]--;
            };
            if (a > b) { longer(a); shorter(b); } else { shorter(b); longer(a); }
            break;
        }
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
        case 6: {  // splice a run of the proof's own bytes in, in place or inserted
            if (m.empty()) break;
            const size_t a = rnd() % m.size(), b = rnd() % src.size(), n = 1 + rnd() % std::min<size_t>(96, src.size() - b);
            if (rnd() & 1) m.insert(m.begin() + a, src.begin() + b, src.begin() + b + n);
            else std::memcpy(&m[a], &src[b], std::min(n, m.size() - a));
            break;
        }
        default: {  // a whole hash inserted behind a random place (a longer path where the place is a path's end)
            const size_t a = m.empty() ? 0 : rnd() % m.size();
            m.insert(m.begin() + a, 32, (uint8_t)1);
            break;
        }
    }
    return m;
}

struct Item {
    std::vector<uint8_t> points, openings, caps, proof;
};

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
        if (n) std::memcpy(dst, &file[off], n);
        off += n;
    };
    uint32_t head[10];
    take(head, sizeof head);
    const uint32_t field = head[0], degree_bits = head[1], rate_bits = head[2], cap_height = head[3], hiding = head[4], no = head[5],
                   nb = head[6], nl = head[7], pow_bits = head[8], nqr = head[9];
    if (no > 4096 || nb > 4096 || nl > 64 || cap_height > 16) return 2;
    std::vector<uint32_t> num_polys(no), blinding(no), sizes(nb), arity(nl);
    take(num_polys.data(), 4 * (size_t)no);
    take(blinding.data(), 4 * (size_t)no);
    take(sizes.data(), 4 * (size_t)nb);
    size_t total = 0;
    for (uint32_t s : sizes) total += s;
    if (total > (1u << 20)) return 2;
    std::vector<uint32_t> polys(2 * total);
    take(polys.data(), 8 * total);
    take(arity.data(), 4 * (size_t)nl);
    gb_challenger_state chs;
    take(&chs, sizeof chs);
    const size_t es = field == GB_GOLDILOCKS ? 8 : 4, D = field == GB_GOLDILOCKS ? 2 : 4, H = field == GB_GOLDILOCKS ? 4 : 8;
    Item good;
    good.points.resize(nb * D * es);
    good.openings.resize(total * D * es);
    good.caps.resize((size_t)no * (H << cap_height) * es);
    take(good.points.data(), good.points.size());
    take(good.openings.data(), good.openings.size());
    take(good.caps.data(), good.caps.size());
    uint64_t proof_len;
    take(&proof_len, 8);
    good.proof.resize(proof_len);
    take(good.proof.data(), proof_len);

    auto alone = [&](const Item& it, const void* proof_ptr) {
        return gb_fri_verify(nullptr, field, degree_bits, rate_bits, cap_height, hiding, num_polys.data(), blinding.data(), no, it.points.data(),
                             sizes.data(), nb, polys.data(), it.openings.data(), it.caps.data(), arity.data(), nl, pow_bits, nqr, &chs, proof_ptr,
                             it.proof.size());
    };
    // the length bytes of the regular proof: behind the layer caps, per query round and tree the row, then the byte and its siblings
    {
        hash_bytes = H * es;
        size_t at = (size_t)nl * (H << cap_height) * es;
        for (uint32_t q = 0; q < nqr; q++)
            for (uint32_t t = 0; t < no + nl; t++) {
                at += t < no ? (size_t)(num_polys[t] + (hiding && blinding[t] ? GB_SALT_SIZE : 0)) * es : (D << arity[t - no]) * es;
                if (at >= good.proof.size()) { std::fprintf(stderr, "the case's proof is shorter than its shape\n"); return 2; }
                length_bytes.push_back(at);
                at += 1 + (size_t)good.proof[at] * hash_bytes;
            }
    }
    static const uint8_t nothing = 0;
    if (alone(good, good.proof.data()) != GB_OK) { std::fprintf(stderr, "the case's own proof: %s\n", gb_last_error(nullptr)); return 1; }

    // batches of four: mutants, and every few rounds the honest item, an empty proof and an item with a word >= p among them
    long host_decided = 0, left_to_device = 0, statuses[3] = {}, wrong_length_at_full_size = 0;
    for (long it = 0; it < iterations; it++) {
        Item batch[4];
        for (int k = 0; k < 4; k++) {
            batch[k] = good;
            batch[k].proof = mutate(good.proof);
        }
        if (it % 5 == 0) batch[1].proof = good.proof;
        if (it % 7 == 0) batch[2].proof.clear();
        if (it % 6 == 0) {   // a word of all ones in the points, the openings or the caps
            std::vector<uint8_t>& v = it % 18 == 0 ? batch[3].points : it % 18 == 6 ? batch[3].openings : batch[3].caps;
            const size_t w = rnd() % (v.size() / es);
            std::memset(&v[w * es], 0xFF, es);
        }
        const void *pts[4], *ops[4], *caps[4], *proofs[4];
        size_t lens[4];
        gb_challenger_state states[4];
        for (int k = 0; k < 4; k++) {
            pts[k] = batch[k].points.data(); ops[k] = batch[k].openings.data(); caps[k] = batch[k].caps.data();
            proofs[k] = batch[k].proof.empty() ? &nothing : batch[k].proof.data();
            lens[k] = batch[k].proof.size();
            states[k] = chs;
        }
        gb_verify_result res[4];
        std::memset(res, 0xAB, sizeof res);
        gb_status s = gb_fri_verify_batch(nullptr, field, degree_bits, rate_bits, cap_height, hiding, num_polys.data(), blinding.data(), no,
                                          sizes.data(), nb, polys.data(), arity.data(), nl, pow_bits, nqr, pts, ops, caps, states, proofs, lens, 4,
                                          0, res);
        if (s != GB_ERR_INVALID || !std::strstr(gb_last_error(nullptr), "null ctx")) {
            std::fprintf(stderr, "the call without a context returned %d (%s)\n", s, gb_last_error(nullptr));
            return 1;
        }
        if (std::memcmp(states, &chs, sizeof chs) != 0) { std::fprintf(stderr, "the call advanced a challenger\n"); return 1; }
        for (int k = 0; k < 4; k++) {
            const gb_status want = alone(batch[k], proofs[k]);
            const std::string text = want == GB_OK ? "" : gb_last_error(nullptr);
            if (want != GB_OK && want != GB_ERR_INVALID && want != GB_ERR_VERIFY) {
                std::fprintf(stderr, "gb_fri_verify returned %d (%s) on a mutated input\n", want, text.c_str());
                return 1;
            }
            statuses[want == GB_OK ? 0 : want == GB_ERR_INVALID ? 1 : 2]++;
            const gb_verify_result& r = res[k];
            if (r.status == GB_ERR_INVALID && r.check == GB_VCHECK_NONE) {   // left to the device: the parser, the proof of work and
                left_to_device++;                                            // the regularity test had nothing to say
                if (lens[k] != good.proof.size()) {
                    std::fprintf(stderr, "iteration %ld: an item of %zu bytes (the shape's: %zu) was left to the device\n", it, lens[k], good.proof.size());
                    return 1;
                }
                const char* host_only[] = {"truncated", "non-canonical", "trailing", "wrong length", "proof of work"};
                for (const char* h : host_only)
                    if (want != GB_OK && text.find(h) != std::string::npos) {
                        std::fprintf(stderr, "iteration %ld: an item gb_fri_verify refuses with '%s' was left to the device\n", it, text.c_str());
                        return 1;
                    }
                continue;
            }
            host_decided++;
            if (lens[k] == good.proof.size() && text.find("wrong length") != std::string::npos) wrong_length_at_full_size++;
            const std::string mine = gb_verify_check_text(r.check);
            // one text per check: gb_fri_verify also says where a word >= p stands, and how a proof shorter than its query rounds is short
            const bool same = text == mine || (r.check == GB_VCHECK_NON_CANONICAL && text.find("non-canonical field element in") == 0) ||
                              (r.check == GB_VCHECK_TRUNCATED && text.find(mine) == 0);
            if ((gb_status)r.status != want || !same) {
                std::fprintf(stderr, "iteration %ld: host stage says %u '%s', gb_fri_verify %d '%s'\n", it, r.status, mine.c_str(), want, text.c_str());
                return 1;
            }
        }
    }
    std::printf("fuzz ok: %ld iterations; host decided %ld, left to the device %ld; gb_fri_verify ok/invalid/verify = %ld/%ld/%ld; "
                "irregular at the shape's length %ld\n",
                iterations, host_decided, left_to_device, statuses[0], statuses[1], statuses[2], wrong_length_at_full_size);
    return 0;
}
