// The word files of tests/host_shim/random_stream.cpp and tests/device/random_stream.hip: their format (random_stream.cpp has the
// table), the records they are parsed into and the one function, run_record, that both programs execute per record - on the
// calling thread or in a kernel.  A range record becomes one element record per element for the device; the host runs it
// through rnd::fill_range as gb_random_elements' callers would.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "random_stream.hpp"

namespace random_case {

using gbk::u32;
using gbk::u64;

enum : u64 { BLOCK = 1, REDUCE = 2, RANGE = 3, ELEMENT = 4 };

struct Record {
    u64 kind, field;
    gbk::rnd::Key key;
    u64 a, b;      // BLOCK: counter; REDUCE: lo, hi; ELEMENT: e; RANGE: first, count
    u64 out_at;    // where its words go
};

inline bool read_words(const char* path, std::vector<uint64_t>* w) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint64_t x;
    while (std::fread(&x, sizeof x, 1, f) == 1) w->push_back(x);
    std::fclose(f);
    return true;
}
inline bool write_words(const char* path, const std::vector<uint64_t>& w) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = w.empty() || std::fwrite(w.data(), sizeof(uint64_t), w.size(), f) == w.size();
    return std::fclose(f) == 0 && ok;
}

// BLOCK -> 8 words, REDUCE / ELEMENT -> 1 word
GB_HD void run_record(const Record& r, uint64_t* out) {
    if (r.kind == BLOCK) {
        u32 w[16];
        gbk::rnd::chacha20_block(r.key, (u32)r.a, w);
        for (int i = 0; i < 8; i++) out[r.out_at + i] = (u64)w[2 * i] | ((u64)w[2 * i + 1] << 32);
    } else if (r.kind == REDUCE) {
        const u32 w[4] = {(u32)r.a, (u32)(r.a >> 32), (u32)r.b, (u32)(r.b >> 32)};
        out[r.out_at] = r.field == 0 ? gbk::rnd::reduce_u128<gbk::GlF>(w) : (u64)gbk::rnd::reduce_u128<gbk::BbF>(w);
    } else if (r.kind == ELEMENT) {
        out[r.out_at] = r.field == 0 ? gbk::rnd::element<gbk::GlF>(r.key, r.a) : (u64)gbk::rnd::element<gbk::BbF>(r.key, r.a);
    }
}

inline bool read_key(const std::vector<uint64_t>& in, size_t* at, gbk::rnd::Key* key) {
    if (*at + 7 > in.size()) return false;
    uint8_t seed[32];
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(in[*at + i / 8] >> (8 * (i % 8)));
    const u32 nonce[3] = {(u32)in[*at + 4], (u32)in[*at + 5], (u32)in[*at + 6]};
    *key = gbk::rnd::make_key(seed, nonce);
    *at += 7;
    return true;
}

// parse the file; `expand_ranges`: a range becomes element records (its range_ok word is written here either way)
inline bool parse(const std::vector<uint64_t>& in, bool expand_ranges, std::vector<Record>* recs, std::vector<uint64_t>* out) {
    size_t at = 0;
    while (at < in.size()) {
        Record r{};
        r.kind = in[at++];
        r.out_at = out->size();
        if (r.kind == BLOCK) {
            if (!read_key(in, &at, &r.key) || at + 1 > in.size()) return false;
            r.a = in[at++];
            if (r.a >> 32) return false;
            out->resize(out->size() + 8);
        } else if (r.kind == REDUCE) {
            if (at + 3 > in.size() || in[at] > 1) return false;
            r.field = in[at]; r.a = in[at + 1]; r.b = in[at + 2];
            at += 3;
            out->resize(out->size() + 1);
        } else if (r.kind == ELEMENT || r.kind == RANGE) {
            if (at + 1 > in.size() || in[at] > 1) return false;
            r.field = in[at++];
            if (!read_key(in, &at, &r.key) || at + (r.kind == RANGE ? 2 : 1) > in.size()) return false;
            r.a = in[at++];
            if (r.kind == ELEMENT) {
                if (r.a >> 34) return false;
                out->resize(out->size() + 1);
            } else {
                r.b = in[at++];
                const bool ok = gbk::rnd::range_ok(r.a, r.b);
                out->push_back(ok ? 1 : 0);
                if (!ok) continue;
                if (r.b > ((u64)1 << 24)) return false;   // a test file, not a bulk generator
                r.out_at = out->size();
                out->resize(out->size() + r.b);
                if (expand_ranges) {
                    for (u64 i = 0; i < r.b; i++) {
                        Record e = r;
                        e.kind = ELEMENT; e.a = r.a + i; e.out_at = r.out_at + i;
                        recs->push_back(e);
                    }
                    continue;
                }
            }
        } else {
            return false;
        }
        recs->push_back(r);
    }
    return true;
}

inline bool on_host(const std::vector<Record>& recs, std::vector<uint64_t>* out) {
    for (const Record& r : recs) {
        if (r.kind != RANGE) { run_record(r, out->data()); continue; }
        if (r.field == 0) {
            gbk::rnd::fill_range<gbk::GlF>(r.key, r.a, r.b, reinterpret_cast<u64*>(out->data()) + r.out_at);
        } else {
            std::vector<u32> v(r.b);
            gbk::rnd::fill_range<gbk::BbF>(r.key, r.a, r.b, v.data());
            for (u64 i = 0; i < r.b; i++) (*out)[r.out_at + i] = v[i];
        }
    }
    return true;
}

template <class Exec>
bool run(const std::vector<uint64_t>& in, std::vector<uint64_t>* out, Exec exec, bool expand_ranges = false) {
    std::vector<Record> recs;
    if (!parse(in, expand_ranges, &recs, out)) return false;
    return exec(recs, out);
}

}  // namespace random_case
