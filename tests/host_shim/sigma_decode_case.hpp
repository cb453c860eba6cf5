// The word file of tests/host_shim/sigma_decode.cpp and tests/device/sigma_decode.hip (the format is in the former), and the loop
// over its cases: the tables of a case are made on the host, `eval` decodes the case's values - on the host or in a kernel.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sigma_decode.hpp"

namespace sigma_case {

inline bool read_words(const char* path, std::vector<uint64_t>* out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint64_t w;
    while (std::fread(&w, sizeof w, 1, f) == 1) out->push_back(w);
    std::fclose(f);
    return true;
}
inline bool write_words(const char* path, const std::vector<uint64_t>& words) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = words.empty() || std::fwrite(words.data(), sizeof(uint64_t), words.size(), f) == words.size();
    return std::fclose(f) == 0 && ok;
}

template <class F>
struct Case {
    gbk::sigma::DlogTablesHost<F> tables;
    std::vector<typename F::T> k_pow_n, k_inv, values;   // device form
};

// cells[2 i], cells[2 i + 1] = col', row' of values[i], or NO_CELL, 0 (row 2^32 - 1 exists at lg = 32)
template <class F>
bool on_host(const Case<F>& c, std::vector<gbk::u32>* cells) {
    const gbk::sigma::DlogTables<F> t = c.tables.view();
    for (size_t i = 0; i < c.values.size(); i++) {
        gbk::u32 col, row;
        if (!gbk::sigma::decode_value<F>(t, c.k_pow_n.data(), c.k_inv.data(), (gbk::u32)c.k_pow_n.size(), c.values[i], &col, &row))
            col = gbk::sigma::NO_CELL, row = 0;
        (*cells)[2 * i] = col;
        (*cells)[2 * i + 1] = row;
    }
    return true;
}

template <class F, class Eval>
bool run(const std::vector<uint64_t>& in, std::vector<uint64_t>* out, Eval eval) {
    typedef typename F::T T;
    size_t pos = 2;
    for (uint64_t k = 0; k < in[1]; k++) {
        if (in.size() - pos < 4) return false;
        const uint64_t lg = in[pos], nr = in[pos + 1], raw = in[pos + 2], count = in[pos + 3];
        pos += 4;
        if (lg > F::TWO_ADICITY || nr > 4096 || count > in.size() - pos || nr > in.size() - pos - count) return false;
        std::vector<T> k_is(nr);
        for (uint64_t j = 0; j < nr; j++) k_is[j] = F::enc(in[pos + j]);
        pos += nr;
        Case<F> c;
        c.tables = gbk::sigma::build_dlog_tables<F>((gbk::u32)lg);
        out->push_back(gbk::sigma::build_coset_tables<F>(k_is.data(), (gbk::u32)nr, (gbk::u32)lg, &c.k_pow_n, &c.k_inv) ? 1 : 0);
        c.values.resize(count);
        for (uint64_t i = 0; i < count; i++) c.values[i] = raw ? (T)in[pos + i] : F::enc(in[pos + i]);
        pos += count;
        std::vector<gbk::u32> cells(2 * count);
        if (!eval(c, &cells)) return false;
        for (uint64_t i = 0; i < count; i++) {
            out->push_back(cells[2 * i] == gbk::sigma::NO_CELL ? ~(uint64_t)0 : (uint64_t)cells[2 * i]);
            out->push_back(cells[2 * i + 1]);
        }
    }
    return pos == in.size();
}

}  // namespace sigma_case
