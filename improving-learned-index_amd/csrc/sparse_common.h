// sparse_common.h -- the float index's handle, shared by its search (sparse.hip) and its
// device builder (sparse_build.hip).
#pragma once

#include "di_common.h"

namespace di {
constexpr int SP_DOCS = 16384;  // docs of one block of the layout (sparse.hip)
}

struct di_sparse {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int64_t n_terms = 0, n_post = 0;
    uint32_t n_docs = 0;
    int nb = 0;
    di::DevBuf pdoc, pimp, term_start, blk_off;
    di::DevBuf ws_q, ws_cu, ws_ck, ws_cn, ws_doc, ws_score, ws_n, ws_key;
    di::Timer timer;
};

namespace di {

// A fresh handle's device, stream and kernel attributes (the current device is `device`).
void sparse_init(di_sparse &sp, int device);

}  // namespace di
