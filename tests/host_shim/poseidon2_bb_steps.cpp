// poseidon2_bb::permute_scaled (csrc/poseidon2_bb.hpp) taken apart on the CPU: its steps - external_layer, sbox7, internal_round, the
// selection in front of round 4 - one call at a time, in the order the header runs them, with the bounds the header states for what
// goes into and comes out of each step checked after every call:
//   external_layer<true>:  words in [0, 2p) in (canonical at the entry), signed words within +-1.03 p out
//   sbox7:                 |x| <= 1.03 p in, a word in (0, 2p) out
//   external_layer<false>: canonical out
//   internal_round:        word 0 a signed word in (-p, p) in and out, words 1..15 below LAZY_MAX in and out
//   the selection:         words 1..15 signed within (-p, p + 2^15)
// At the end the words must EQUAL those of poseidon2_bb::permute_scaled on the same input (a drift between this program's step order
// and the header's shows up here) and, through canonical_out, the host mirror's (csrc/poseidon2_bb_host.hpp).
// argv[1]: a file of u32 records {16 canonical input words, place, word index, word}: states pulled back from chosen round words
// (tests/permutation_states.py).  place = 2 * round + (0: s-box input, 1: s-box output), rounds 0..20; the step's word `index` must be
// congruent to `word` mod p (index = 0xFFFFFFFF: no such check) - which checks the scale sequence the Python model restates.
// argv[2]: the number of random states that follow.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "poseidon2_bb.hpp"
#include "poseidon2_bb_host.hpp"

typedef uint32_t u32;
static const long long P = bb::P, SLIM = 2073663898LL;   // floor(1.03 p)
static long bad = 0, bound_checks = 0, place_checks = 0;

static void fail(const char* what, long state, int step, int word, u32 v) {
    if (++bad <= 12) printf("state %ld step %d word %d: %s (%08x)\n", state, step, word, what, v);
}
static u32 residue(u32 signed_word) {
    const long long r = (long long)(int)signed_word % P;
    return (u32)(r < 0 ? r + P : r);
}
struct Probe {
    long state;
    u32 place, index, word;
    // `place` reached with the state `s`; as_signed: the words are signed
    void at(u32 here, const u32* s, bool as_signed) const {
        if (here != place || index == 0xFFFFFFFFu) return;
        place_checks++;
        const u32 got = as_signed ? residue(s[index]) : s[index] % bb::P;
        if (got != word % bb::P) fail("the chosen word did not arrive", state, (int)here, (int)index, s[index]);
    }
};

static void all_signed(const u32* s, int from, long long lo, long long hi, const char* what, long state, int step) {
    for (int i = from; i < 16; i++) {
        bound_checks++;
        const long long v = (int)s[i];
        if (v < lo || v > hi) fail(what, state, step, i, s[i]);
    }
}
static void all_below(const u32* s, int from, unsigned long long lim, bool positive, const char* what, long state, int step) {
    for (int i = from; i < 16; i++) {
        bound_checks++;
        if (s[i] >= lim || (positive && s[i] == 0)) fail(what, state, step, i, s[i]);
    }
}

static void run(const u32* in, long state, const Probe& probe) {
    using namespace poseidon2_bb;
    u32 s[16], whole[16], ref[16];
    for (int i = 0; i < 16; i++) { s[i] = bb::to_mont(in[i]); whole[i] = s[i]; ref[i] = in[i]; }
    all_below(s, 0, bb::P, false, "entry: not canonical", state, -1);
    external_layer<true>(s, PLAN.ext[0]);
    for (int r = 0; r < 4; r++) {
        all_signed(s, 0, -SLIM, SLIM, "s-box input outside +-1.03 p", state, 2 * r);
        probe.at(2 * r, s, true);
        for (int i = 0; i < 16; i++) s[i] = sbox7(s[i]);
        all_below(s, 0, 2ULL * bb::P, true, "s-box output outside (0, 2p)", state, 2 * r + 1);
        probe.at(2 * r + 1, s, false);
        if (r < 3) external_layer<true>(s, PLAN.ext[r + 1]);
        else external_layer(s, ZERO16);
    }
    all_below(s, 0, bb::P, false, "external_layer<false>: not canonical", state, 7);
    s[0] = bb::add(s[0], PLAN.in[0]);
    for (int r = 0; r < 13; r++) {
        const int place = 2 * (4 + r);
        bound_checks++;
        if ((long long)(int)s[0] <= -P || (long long)(int)s[0] >= P) fail("internal round: word 0 outside (-p, p)", state, place, 0, s[0]);
        all_below(s, 1, LAZY_MAX, false, "internal round: lazy word not below LAZY_MAX", state, place);
        probe.at(place, s, true);
        const u32 y[16] = {sbox7(s[0])};   // the round's s-box output (internal_round computes it inside); words 1..15 are not probed here
        bound_checks++;
        if (y[0] == 0 || y[0] >= 2ULL * bb::P) fail("internal s-box output outside (0, 2p)", state, place + 1, 0, y[0]);
        probe.at(place + 1, y, false);
        internal_round(s, PLAN.in[r + 1], PLAN.sumc[r]);
    }
    {   // what leaves the last internal round
        bound_checks++;
        if ((long long)(int)s[0] <= -P || (long long)(int)s[0] >= P) fail("after the internal rounds: word 0 outside (-p, p)", state, 33, 0, s[0]);
        all_below(s, 1, LAZY_MAX, false, "after the internal rounds: lazy word not below LAZY_MAX", state, 33);
    }
    for (int i = 1; i < 16; i++) {   // the selection in front of round 4 (permute_scaled)
        const u32 t = s[i] - bb::P;
        s[i] = (t < s[i] ? t : s[i]) + (PLAN.ext4[i] - bb::P);
    }
    all_signed(s, 1, -(P - 1), P + (1 << 15) - 1, "selection: word outside (-p, p + 2^15)", state, 34);
    for (int r = 4; r < 8; r++) {
        const int place = 2 * (13 + r);
        all_signed(s, 0, -SLIM, SLIM, "s-box input outside +-1.03 p", state, place);
        probe.at(place, s, true);
        for (int i = 0; i < 16; i++) s[i] = sbox7(s[i]);
        all_below(s, 0, 2ULL * bb::P, true, "s-box output outside (0, 2p)", state, place + 1);
        probe.at(place + 1, s, false);
        if (r < 7) external_layer<true>(s, PLAN.ext[r + 1]);
        else external_layer(s, ZERO16);
    }
    all_below(s, 0, bb::P, false, "external_layer<false>: not canonical", state, 42);
    permute_scaled(whole);
    poseidon2_bb_host::permute(ref);
    for (int i = 0; i < 16; i++) {
        if (s[i] != whole[i]) fail("the steps differ from permute_scaled", state, 42, i, s[i]);
        if (canonical_out(s[i]) != ref[i]) fail("canonical_out differs from the host mirror", state, 43, i, s[i]);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: poseidon2_bb_steps <states file> <random states>\n"); return 2; }
    std::vector<u32> rec;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { printf("cannot read %s\n", argv[1]); return 2; }
        u32 buf[19 * 64];
        for (size_t n; (n = fread(buf, sizeof(u32), 19 * 64, f)) > 0;) rec.insert(rec.end(), buf, buf + n);
        fclose(f);
        if (rec.size() % 19) { printf("%s: not a whole number of records\n", argv[1]); return 2; }
    }
    const long nfile = (long)(rec.size() / 19), nrandom = atol(argv[2]);
    for (long t = 0; t < nfile; t++) {
        const u32* r = &rec[19 * t];
        bool ok = r[16] <= 41 && (r[17] < 16 || r[17] == 0xFFFFFFFFu);
        ok = ok && (r[16] < 8 || r[16] > 33 || r[17] == 0 || r[17] == 0xFFFFFFFFu);   // inside the internal rounds only word 0 is at the common scale
        for (int i = 0; i < 16; i++) ok = ok && r[i] < bb::P;
        if (!ok) { printf("record %ld is malformed\n", t); return 2; }
        run(r, t, Probe{t, r[16], r[17], r[18]});
    }
    std::mt19937_64 rng(11);
    for (long t = 0; t < nrandom; t++) {
        u32 in[16];
        for (int i = 0; i < 16; i++) {
            in[i] = (u32)(rng() % bb::P);
            if (t % 9 == 0) in[i] = bb::P - 1 - (u32)(rng() % 3);
            if (t % 13 == 0) in[i] = (i & 1) ? bb::P - 1 : 0;
        }
        run(in, nfile + t, Probe{nfile + t, 0, 0xFFFFFFFFu, 0});
    }
    printf("states=%ld bound_checks=%ld place_checks=%ld mismatches=%ld\n", nfile + nrandom, bound_checks, place_checks, bad);
    return bad != 0;
}
