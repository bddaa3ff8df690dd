// term_table.cpp -- di_term_table_*: the host side of the device index builder's route.
//
// The terms of an encode step arrive as the tokenizer workers send them -- one UTF-8 blob
// and byte offsets -- and leave as uint32 ids in order of first appearance, the ids
// di_index_builder_append stores.  After di_index_builder_quantize has counted the kept
// postings per id, di_term_table_rows numbers the terms that kept one in ascending byte
// order of their UTF-8: code-point order, Python's sorted() on str, the order of
// vocab.txt (create.py:24-27).
//
// Precondition, checked at interning: the text route writes a term into
// ', '.join(f'{term}: {impact}') and parses it back with line.strip().split(', ') and
// t.strip().split(': ') (quantize.py:21-22, deep_impact_collection.py:20-27).  A term
// that would not come back as itself -- empty, with whitespace at either end, holding
// ', ', ': ' or a line break -- is refused here, so both routes stay byte-equal.
#include <algorithm>
#include <cstring>
#include <numeric>

#include "di_common.h"
#include "pytext.h"
#include "term_table.h"

namespace {

using namespace di;

constexpr size_t kBlock = size_t(1) << 20;

std::string_view store(di_term_table *t, std::string_view x) {
    if (x.size() > kBlock / 4) {  // a long term: a block of its own, the open one stays open
        t->blocks.emplace_back(new char[x.size()]);
        char *p = t->blocks.back().get();
        std::memcpy(p, x.data(), x.size());
        return {p, x.size()};
    }
    if (x.size() > t->block_left) {
        t->blocks.emplace_back(new char[kBlock]);
        t->block_at = t->blocks.back().get();
        t->block_left = kBlock;
    }
    char *p = t->block_at;
    std::memcpy(p, x.data(), x.size());
    t->block_at += x.size();
    t->block_left -= x.size();
    return {p, x.size()};
}

void check_term(std::string_view x, int64_t i) {
    const char *why = nullptr;
    if (x.empty()) why = "is empty";
    else if (py::strip(x).size() != x.size()) why = "has whitespace at an end";
    else if (x.find(", ") != std::string_view::npos) why = "holds ', '";
    else if (x.find(": ") != std::string_view::npos) why = "holds ': '";
    else if (x.find('\n') != std::string_view::npos || x.find('\r') != std::string_view::npos)
        why = "holds a line break";
    DI_REQUIRE(!why, DI_EFORMAT,
               "term %lld '%.*s' %s: the impact TSV would not parse back to it; build this "
               "collection by the text route (index, quantize, inverted_index)",
               (long long)i, (int)std::min<size_t>(x.size(), 200), x.data(), why);
}

// The names of the entries of di_term_table_rows_pairwise, compared without being built:
// entry e < n_terms is term e, entry n_terms + u is term[first[u]] + '|' + term[second[u]].
struct PairNames {
    const di_term_table *t;
    const uint32_t *first, *second;
    size_t n_terms;
    static constexpr std::string_view kBar{"|", 1};

    int parts(uint64_t e, std::string_view out[3]) const {
        if (e < n_terms) {
            out[0] = t->terms[(size_t)e];
            return 1;
        }
        out[0] = t->terms[first[e - n_terms]];
        out[1] = kBar;
        out[2] = t->terms[second[e - n_terms]];
        return 3;
    }
    // < 0, 0, > 0 as unsigned bytes: code-point order for valid UTF-8
    int compare(uint64_t a, uint64_t b) const {
        std::string_view pa[3], pb[3];
        const int na = parts(a, pa), nb = parts(b, pb);
        int ia = 0, ib = 0;
        size_t oa = 0, ob = 0;
        for (;;) {
            while (ia < na && oa == pa[ia].size()) ++ia, oa = 0;
            while (ib < nb && ob == pb[ib].size()) ++ib, ob = 0;
            if (ia == na || ib == nb) return (ia == na ? 0 : 1) - (ib == nb ? 0 : 1);
            const size_t n = std::min(pa[ia].size() - oa, pb[ib].size() - ob);
            const int c = std::memcmp(pa[ia].data() + oa, pb[ib].data() + ob, n);
            if (c) return c;
            oa += n;
            ob += n;
        }
    }
    std::string name(uint64_t e) const {
        std::string_view p[3];
        const int n = parts(e, p);
        std::string s;
        for (int i = 0; i < n; ++i) s.append(p[i].data(), p[i].size());
        return s;
    }
};

}  // namespace

extern "C" {

int di_term_table_create(di_term_table **out) {
    return guard([&] {
        DI_REQUIRE(out, DI_EINVAL, "null output");
        *out = new di_term_table;
    });
}

int di_term_table_intern(di_term_table *t, const char *blob, const int64_t *term_off, int64_t n,
                         uint32_t *ids) {
    return guard([&] {
        DI_REQUIRE(t && n >= 0 && (n == 0 || (blob && term_off && ids)), DI_EINVAL, "bad argument");
        for (int64_t i = 0; i < n; ++i) {  // before anything changes
            DI_REQUIRE(term_off[i] >= 0 && term_off[i + 1] >= term_off[i], DI_EINVAL,
                       "term_off not monotone at %lld", (long long)i);
            check_term({blob + term_off[i], (size_t)(term_off[i + 1] - term_off[i])}, i);
        }
        for (int64_t i = 0; i < n; ++i) {
            const std::string_view x(blob + term_off[i], (size_t)(term_off[i + 1] - term_off[i]));
            auto it = t->ids.find(x);
            if (it == t->ids.end()) {
                DI_REQUIRE(t->terms.size() < 0xFFFFFFFFull, DI_ERANGE, "more than 2^32 terms");
                const std::string_view kept = store(t, x);
                it = t->ids.emplace(kept, (uint32_t)t->terms.size()).first;
                t->terms.push_back(kept);
            }
            ids[i] = it->second;
        }
    });
}

int di_term_table_info(const di_term_table *t, int64_t *n_terms, int64_t *n_bytes) {
    return guard([&] {
        DI_REQUIRE(t, DI_EINVAL, "null handle");
        if (n_terms) *n_terms = (int64_t)t->terms.size();
        if (n_bytes) {
            int64_t b = 0;
            for (auto x : t->terms) b += (int64_t)x.size();
            *n_bytes = b;
        }
    });
}

int di_term_table_export(const di_term_table *t, char *blob, int64_t *term_off) {
    return guard([&] {
        DI_REQUIRE(t && term_off && (blob || t->terms.empty()), DI_EINVAL, "bad argument");
        int64_t at = 0;
        for (size_t i = 0; i < t->terms.size(); ++i) {
            term_off[i] = at;
            if (!t->terms[i].empty()) std::memcpy(blob + at, t->terms[i].data(), t->terms[i].size());
            at += (int64_t)t->terms[i].size();
        }
        term_off[t->terms.size()] = at;
    });
}

int di_term_table_rows(const di_term_table *t, const int64_t *term_count, int32_t *term_row,
                       int64_t *n_rows) {
    return guard([&] {
        DI_REQUIRE(t && n_rows && (t->terms.empty() || (term_count && term_row)), DI_EINVAL,
                   "bad argument");
        std::vector<uint32_t> kept;
        for (size_t i = 0; i < t->terms.size(); ++i) {
            term_row[i] = -1;
            if (term_count[i] > 0) kept.push_back((uint32_t)i);
        }
        DI_REQUIRE(kept.size() <= (size_t)INT32_MAX, DI_ERANGE, "more than 2^31 kept terms");
        // std::string_view compares as unsigned bytes: code-point order for valid UTF-8
        std::sort(kept.begin(), kept.end(),
                  [&](uint32_t a, uint32_t b) { return t->terms[a] < t->terms[b]; });
        for (size_t r = 0; r < kept.size(); ++r) term_row[kept[r]] = (int32_t)r;
        *n_rows = (int64_t)kept.size();
    });
}

int di_term_table_rows_pairwise(const di_term_table *t, const int64_t *term_count,
                                int64_t n_pair_terms, const uint32_t *first_id,
                                const uint32_t *second_id, int32_t *term_row, int64_t *n_rows) {
    return guard([&] {
        DI_REQUIRE(t && n_rows && n_pair_terms >= 0 && term_row &&
                       (t->terms.empty() || term_count) &&
                       (n_pair_terms == 0 || (first_id && second_id)),
                   DI_EINVAL, "bad argument");
        const size_t n_terms = t->terms.size();
        for (int64_t u = 0; u < n_pair_terms; ++u)
            DI_REQUIRE(first_id[u] < n_terms && second_id[u] < n_terms, DI_EINVAL,
                       "pair %lld: a term id is not below n_terms = %lld", (long long)u,
                       (long long)n_terms);
        // an entry: a single term id, or n_terms + u
        std::vector<uint64_t> single, pairs((size_t)n_pair_terms);
        for (size_t i = 0; i < n_terms; ++i) {
            term_row[i] = -1;
            if (term_count[i] > 0) single.push_back(i);
        }
        for (int64_t u = 0; u < n_pair_terms; ++u) {
            term_row[n_terms + (size_t)u] = -1;
            pairs[(size_t)u] = n_terms + (uint64_t)u;
        }
        DI_REQUIRE(single.size() + pairs.size() <= (size_t)INT32_MAX, DI_ERANGE,
                   "more than 2^31 kept terms");
        const PairNames names{t, first_id, second_id, n_terms};
        auto less = [&](uint64_t a, uint64_t b) { return names.compare(a, b) < 0; };
        std::sort(single.begin(), single.end(), less);
        // the pair names: sorted in contiguous chunks on the host threads, then merged
        const int64_t P = n_pair_terms;
        const int C = (int)std::min<int64_t>(host_threads(), std::max<int64_t>(P / 4096, 1));
        parallel_for_threads(C, C, [&](int64_t lo, int64_t hi, int) {
            for (int64_t c = lo; c < hi; ++c)
                std::sort(pairs.begin() + P * c / C, pairs.begin() + P * (c + 1) / C, less);
        });
        for (int w = 1; w < C; w *= 2) {
            const int merges = (C + 2 * w - 1) / (2 * w);
            parallel_for_threads(merges, merges, [&](int64_t lo, int64_t hi, int) {
                for (int64_t g = lo; g < hi; ++g) {
                    const int a = (int)g * 2 * w, m = std::min(a + w, C), e = std::min(a + 2 * w, C);
                    std::inplace_merge(pairs.begin() + P * a / C, pairs.begin() + P * m / C,
                                       pairs.begin() + P * e / C, less);
                }
            });
        }
        std::vector<uint64_t> all(single.size() + pairs.size());
        std::merge(single.begin(), single.end(), pairs.begin(), pairs.end(), all.begin(), less);
        for (size_t r = 0; r + 1 < all.size(); ++r)
            if (names.compare(all[r], all[r + 1]) == 0) {
                const std::string x = names.name(all[r]);
                DI_REQUIRE(false, DI_EFORMAT,
                           "two kept terms are named '%.200s' (a pair name equals another "
                           "entry's): the text route merges them into one vocabulary line; build "
                           "this collection by the text route (index, quantize, inverted_index)",
                           x.c_str());
            }
        for (size_t r = 0; r < all.size(); ++r) term_row[all[r]] = (int32_t)r;
        *n_rows = (int64_t)all.size();
    });
}

int di_term_table_destroy(di_term_table *t) {
    return guard([&] { delete t; });
}

}  // extern "C"
