// index_layout.h -- the scorer's blocked device layout built on the device
// (index_layout.hip) for di_index_create_device (index.hip).  gfx950 only.
#pragma once

#include "di_common.h"

namespace di {

// The layout constants the builder shares with the scorer (index.hip asserts they are
// index_score.h's MAX_BLOCK_DOCS, WSEG, WLONG_MIN and POST_X).
constexpr int IL_BLOCK_DOCS = 32768;
constexpr int IL_WSEG = 16;
constexpr int IL_WLONG_MIN = 128;
constexpr uint32_t IL_POST_X = (uint32_t)IL_BLOCK_DOCS << 10;

// What build_index() leaves in a di_index: its ten arrays (filled in place) and scalars.
struct IndexLayout {
    DevBuf *post, *post_flat, *tb_start, *eblk, *epos, *seg, *lid, *wmeta, *emax, *wmax;
    int64_t n_post = 0, n_ent = 0, n_long = 0;
    uint32_t n_docs = 0, doc_lo = 0;
    int nb = 0, block_docs = 0;
    bool has_flat = false;
};

// build_index() of index.hip on the device, byte for byte: term_off[n_terms + 1], pdoc and
// pval are device arrays.  Runs on s and waits for it; its scratch is freed at return.
void build_layout_device(const int64_t *term_off, int64_t n_terms, const uint32_t *pdoc,
                         const uint8_t *pval, uint32_t doc_lo, uint32_t doc_hi, hipStream_t s,
                         bool timing, Timer &timer, IndexLayout &out);

}  // namespace di
