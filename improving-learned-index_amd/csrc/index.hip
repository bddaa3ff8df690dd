// index.hip -- the quantized inverted index's host side for MI355X (gfx950): the
// di_index handle, the host layout builders (build_index, build_packed), reference
// loading and every di_index_* entry point.  The scorer's device code and its launcher
// are index_score.hip (index_score.h), the top-k merge is topk_merge.hip.
//
// Device layout ("doc-blocked, impact-ordered postings"):
//   docs of a shard are cut into nb = ceil(n_docs / 32768) equal blocks (a multiple
//   of 64 docs each, at most 32768); every term's postings are grouped by block
//   (block-major; inside a block by impact class, bank-dealt).  One posting = one
//   u32: (doc_in_block << 8) | value.  A sparse term -> block table locates the
//   (term, block) sublists (SubIndex).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <memory>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "di_common.h"
#include "index_layout.h"
#include "index_score.h"
#include "topk_common.h"
#include "topk_merge.h"

using namespace di;

struct di_index {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int64_t n_terms = 0, n_post = 0, n_ent = 0, n_long = 0;
    uint32_t n_docs = 0, doc_lo = 0;  // shard [doc_lo, doc_lo + n_docs)
    int nb = 0, block_docs = 0;
    int min_cls = 7;                 // impact-class prefix scored (7 = every posting: exact)
    float bm_factor = 0.0f;          // block-max skipping: 0 off, 1 exact, > 1 approximate
    // postings and the sparse (term, block) entries (SubIndex)
    DevBuf post, tb_start, eblk, epos, seg, lid, wmeta, emax, wmax;
    DevBuf post_flat;      // exact scoring: the per-wave runs dealt flat (build_index)
    bool has_flat = false;
    // the posting array a search reads: flat for exact scoring, class-ordered under pruning
    const uint32_t *post_for(int mc) const {
        return has_flat && mc >= 7 ? post_flat.as<uint32_t>() : post.as<uint32_t>();
    }
    DevBuf ws_q, ws_cu, ws_ck, ws_cn, ws_doc, ws_score, ws_n, ws_key, ws_thr;
    DevBuf ws_rec;  // ItemRec per (item, term slot): item_setup_kernel -> score_blocks
    DevBuf ws_long;  // score_blocks -> score_long_kernel: the batch has long queries
    DevBuf bm_stat;  // block-max statistics: u64 {segments evaluated, segments skipped}
    DevBuf ws_border;  // block-max: each query's block order (block_order_kernel)
    DevBuf ws_tq;      // block-max: each query's running threshold (one word)
    // packed (block-compressed) postings, built by di_index_set_packed (SubIndex pk_*)
    DevBuf pk_fs, pk_fwt, pk_fh, pk_data;
    bool pk_built = false, packed = false;
    int64_t pk_frames = 0, pk_bytes = 0;
    // per-query threshold shared across blocks: -1 = auto (on from 8 blocks: at 4 blocks it
    // measured 2.31 vs 2.14 ms per 6980-query batch, at 34 / 269 blocks 16.9 vs 19.5 and
    // 130 vs 161 ms, merge 0.5 vs 7.1 and 1.4 vs 74 ms); DI_SCORE_THRESHOLD=0 / 1 forces
    int shared_thr = -1;
    bool block_order = false;  // DI_BLOCK_ORDER=1: block-max items in per-query bound order
    // threshold refresh schedule (score_item): with the shared threshold, the items of
    // blocks b < tq_first and b % tq_every == 0 read the query's histogram, the others
    // the running word qtq (DI_TQ_EVERY / DI_TQ_FIRST; tq_every 1: every item reads it,
    // as before round 6).  8 / 4 from the sweep (profiles/round6_d_tq_sweep_*.json, one
    // box): 8.8 M skewed docs 94.0 -> 102.7 k q/s (score_blocks 70.7 -> 64.0 ms per
    // 6980-query batch), 1.1 M docs 14.47 -> 14.13-14.23 ms; 4 / 0 and 8 / 0 were slower
    // at 1.1 M (their stale thresholds overflow more sweeps), 16 / 4 and 32 / 8 no faster.
    int tq_every = 8, tq_first = 4;
    int ablate = 0;  // DI_PROFILE_ABLATE: profiling and A/B bits, the AB_* enum of index_score.h
    Timer timer;

    // Few blocks (2..7, no shared qhist threshold): the emit-above selection (score_item)
    // lists up to 2 k keys per (query, block) against the running threshold qtq
    // (AB_NO_EMIT_ABOVE: off, A/B).  One predicate for search and reserve.
    bool few_blocks(int k) const {
        return nb >= 2 && nb < 8 && shared_thr != 1 && 2 * k <= 2048 && !(ablate & AB_NO_EMIT_ABOVE);
    }
    int list_cap(int k) const { return few_blocks(k) ? 2 * k : k; }

    SubIndex sub(bool with_packed = false) const {
        const bool pk = with_packed && packed && pk_built;
        return SubIndex{tb_start.as<uint32_t>(), eblk.as<uint16_t>(), epos.as<uint32_t>(),
                        seg.as<uint16_t>(), lid.as<uint32_t>(), wmeta.as<uint16_t>(),
                        emax.as<uint8_t>(), wmax.as<uint8_t>(),
                        pk ? pk_fs.as<uint32_t>() : nullptr, pk ? pk_fwt.as<uint16_t>() : nullptr,
                        pk ? pk_fh.as<uint4>() : nullptr, pk ? pk_data.as<uint32_t>() : nullptr};
    }
};

namespace {

template <class T>
void upload(DevBuf &d, const std::vector<T> &h) {
    d.reserve(std::max<size_t>(h.size() * sizeof(T), 16));
    if (!h.empty()) DI_HIP(hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
}

// The device index of postings given in the reference file order (term-major, value
// desc / doc asc): the shard's docs in nb equal blocks; per term only the blocks it has
// postings in get an entry (the sparse term -> block table: a multi-million-term
// vocabulary costs its entries, not n_terms x nb).  Every pass runs over term ranges on
// host_threads() threads (a term owns disjoint output ranges); the result does not
// depend on the thread count.
void build_index(di_index *ix, const int64_t *term_off, int64_t n_terms, const uint32_t *pdoc,
                 const uint8_t *pval, uint32_t doc_lo, uint32_t doc_hi) {
    DI_REQUIRE(n_terms >= 0, DI_EINVAL, "n_terms < 0");
    DI_REQUIRE(n_terms < (int64_t)0xFFFFFFFF, DI_ERANGE, "n_terms %lld >= 2^32",
               (long long)n_terms);
    DI_REQUIRE(term_off[0] >= 0, DI_EINVAL, "term_off[0] < 0");
    for (int64_t t = 0; t < n_terms; ++t)
        DI_REQUIRE(term_off[t + 1] >= term_off[t], DI_EINVAL, "term_off not monotone at %lld",
                   (long long)t);
    if (doc_hi == 0) {
        uint32_t mx = 0;
        bool any = false;
        for (int64_t p = term_off[0]; p < term_off[n_terms]; ++p) {
            mx = std::max(mx, pdoc[p]);
            any = true;
        }
        doc_hi = any ? mx + 1 : doc_lo;
    }
    DI_REQUIRE(doc_hi >= doc_lo, DI_EINVAL, "doc_hi < doc_lo");
    const uint32_t nd = doc_hi - doc_lo;
    const int nb = (int)((nd + MAX_BLOCK_DOCS - 1) / MAX_BLOCK_DOCS);
    DI_REQUIRE(nb <= 65535, DI_ERANGE, "%u docs in one shard: more than 65535 blocks", nd);
    // equal blocks (no small tail block costing a whole workgroup per query)
    const uint32_t bd =
        nb ? (uint32_t)std::min<uint64_t>(MAX_BLOCK_DOCS, ((nd + nb - 1) / nb + 63) / 64 * 64)
           : (uint32_t)MAX_BLOCK_DOCS;
    ix->n_terms = n_terms;
    ix->n_docs = nd;
    ix->doc_lo = doc_lo;
    ix->nb = nb;
    ix->block_docs = (int)bd;
    const uint32_t NO = 0xFFFFFFFFu;

    // pass 1: per term, kept postings and the blocks holding them
    std::vector<uint32_t> n_kept((size_t)n_terms + 1, 0), n_ent_t((size_t)n_terms + 1, 0);
    parallel_for(n_terms, [&](int64_t t0, int64_t t1, int) {
        std::vector<uint32_t> cnt((size_t)std::max(nb, 1), 0);
        std::vector<int> touched;
        for (int64_t t = t0; t < t1; ++t) {
            uint32_t kept = 0;
            touched.clear();
            for (int64_t p = term_off[t]; p < term_off[t + 1]; ++p) {
                if (pval[p] == 0) break;  // inverted_index.py:50-51
                const uint32_t d = pdoc[p];
                if (d < doc_lo || d >= doc_hi) continue;
                const int b = (int)((d - doc_lo) / bd);
                if (cnt[b]++ == 0) touched.push_back(b);
                ++kept;
            }
            for (int b : touched) cnt[b] = 0;
            n_kept[t] = kept;
            n_ent_t[t] = (uint32_t)touched.size();
        }
    });
    std::vector<uint32_t> tb_start((size_t)n_terms + 1, 0);
    std::vector<uint64_t> tstart((size_t)n_terms + 1, 0);
    uint64_t total = 0, n_ent = 0;
    for (int64_t t = 0; t < n_terms; ++t) {
        tstart[t] = total;
        tb_start[t] = (uint32_t)n_ent;
        total += n_kept[t];
        n_ent += n_ent_t[t];
        DI_REQUIRE(total < NO && n_ent < NO, DI_ERANGE,
                   "more than 2^32 postings / (term, block) entries in one shard");
    }
    tstart[n_terms] = total;
    tb_start[n_terms] = (uint32_t)n_ent;
    std::vector<uint32_t>().swap(n_kept);
    std::vector<uint32_t>().swap(n_ent_t);
    ix->n_post = (int64_t)total;
    ix->n_ent = (int64_t)n_ent;

    // pass 2: the entries (block, start) and the postings placed by block (stable: the
    // reference order inside each sublist)
    std::vector<uint16_t> eblk((size_t)std::max<uint64_t>(n_ent, 1));
    std::vector<uint32_t> epos((size_t)n_ent + 1);
    std::vector<uint32_t> packed((size_t)std::max<uint64_t>(total, 4));
    parallel_for(n_terms, [&](int64_t t0, int64_t t1, int) {
        std::vector<uint32_t> cur((size_t)std::max(nb, 1), 0);
        std::vector<int> touched;
        for (int64_t t = t0; t < t1; ++t) {
            touched.clear();
            for (int64_t p = term_off[t]; p < term_off[t + 1]; ++p) {
                if (pval[p] == 0) break;
                const uint32_t d = pdoc[p];
                if (d < doc_lo || d >= doc_hi) continue;
                const int b = (int)((d - doc_lo) / bd);
                if (cur[b]++ == 0) touched.push_back(b);
            }
            std::sort(touched.begin(), touched.end());
            uint32_t run = (uint32_t)tstart[t];
            uint32_t e = tb_start[t];
            for (int b : touched) {
                eblk[e] = (uint16_t)b;
                epos[e++] = run;
                const uint32_t c = cur[b];
                cur[b] = run;  // now the block's write cursor
                run += c;
            }
            for (int64_t p = term_off[t]; p < term_off[t + 1]; ++p) {
                if (pval[p] == 0) break;
                const uint32_t d = pdoc[p];
                if (d < doc_lo || d >= doc_hi) continue;
                const uint32_t r = d - doc_lo;
                packed[cur[r / bd]++] = ((r % bd) << 8) | pval[p];
            }
            for (int b : touched) cur[b] = 0;
        }
    });
    epos[n_ent] = (uint32_t)total;

    // long sublists (>= WLONG_MIN postings) get ids in entry order (DI_WLONG_MIN
    // overrides the threshold: layout A/B only, any value is exact)
    uint32_t wlong_min = WLONG_MIN;
    if (const char *e = std::getenv("DI_WLONG_MIN")) wlong_min = (uint32_t)std::max(1, std::atoi(e));
    std::vector<uint32_t> lid((size_t)std::max<uint64_t>(n_ent, 1), NO);
    uint32_t n_long = 0;
    for (uint64_t e = 0; e < n_ent; ++e)
        if (epos[e + 1] - epos[e] >= wlong_min) lid[e] = n_long++;
    ix->n_long = n_long;

    // pass 3: order inside every sublist, the impact-class offsets and the block max.
    // Postings are grouped by impact class c = 7 - floor(log2 value) (class 0 = values
    // 128..255, ..., class 7 = value 1), classes in order, so that "every posting with
    // value >= 2^(7-c)" is a prefix of the sublist: seg[8e + c] = its length
    // (di_index_set_min_impact prunes with it; class 7 = the whole sublist = exact).
    // Inside a class, postings are dealt from their 32 LDS bank buckets (doc_in_block
    // mod 32, distinct banks per aligned 32-posting block where the class allows, see
    // emit_group): the scorer's lanes read consecutive postings and update
    // acc[doc_in_block], and a 32-lane group of a ds_read_b32 / ds_write_b32 conflicts
    // on equal banks.  Any order is exact: a doc occurs once per term, and its key (first term,
    // value there) does not depend on the order inside the term.
    // Long sublists are laid out by wave segment first: wave w of the scorer owns the
    // block's docs [w S, (w + 1) S), S = ceil(bd / 16), and its postings of the sublist
    // form one run (classes in order, bank-dealt inside), so that no two waves touch one
    // doc.  wmeta[lid * 128 + 8 w + c] = end of class c of segment w (offset in the
    // sublist).  emax[e] = the sublist's largest value (block-max metadata).
    std::vector<uint16_t> seg((size_t)std::max<uint64_t>(n_ent * 8, 8), 0);
    std::vector<uint16_t> wmeta((size_t)std::max<uint32_t>(n_long, 1) * WSEG * 8, 0);
    std::vector<uint8_t> emax((size_t)std::max<uint64_t>(n_ent, 1), 0);
    std::vector<uint8_t> wmax((size_t)std::max<uint32_t>(n_long, 1) * WSEG, 0);
    auto cls_of = [](uint32_t w) { return 7 - (31 - __builtin_clz(w & 255u)); };
    auto bank_of = [](uint32_t w) { return (w >> 8) & 31u; };  // doc_in_block mod 32
    const uint32_t S = (bd + WSEG - 1) / WSEG;
    // The scorer's 16-byte loads (scatter_load wide) give a 32-lane group of one LDS
    // update the positions 4 L + k (L < 32) of an aligned 128-position block; DI_DEAL_X4=0
    // deals for the 4-byte loads' lane-consecutive groups instead (A/B).
    bool deal_x4 = true;
    if (const char *e = std::getenv("DI_DEAL_X4")) deal_x4 = std::atoi(e) != 0;
    // A second posting array for exact scoring, `flat`: the per-wave runs of long
    // sublists dealt without the impact-class order.  Class boundaries leave each 32-lane
    // set of a run with ~1.1 repeated LDS banks (a simulation of this dealing over i.i.d.
    // runs of 300-1200 postings, tools/deal_sim.py), flat runs 0.26-0.68, and the scatter's
    // reads conflict accordingly (PMC at 100 k docs: 0.45 of its LDS cycles).  Impact
    // pruning keeps the class-ordered array, whose prefixes it scores.  Same offsets in both
    // (a run is the same postings in another order); 4 B per posting more in HBM.
    // DI_DEAL_CLASSES=1: one array, class-ordered (A/B).
    bool flat_runs = true;
    if (const char *e = std::getenv("DI_DEAL_CLASSES")) flat_runs = std::atoi(e) == 0;
    std::vector<uint32_t> flat;
    if (flat_runs) flat.resize(packed.size());
    parallel_for(n_terms, [&](int64_t t0, int64_t t1, int) {
        std::vector<uint32_t> grp, tmp, bk, seg_in, cls_cnt(8), cls_pos(8), bucket_cnt(32),
            head(32), fill(32);
        // one group (any order in): classes in order (stable), each dealt round-robin
        // from its 32 LDS bank buckets into packed[o..]; cum[c] = end of class c
        // relative to the sublist start s0
        // one_class: dealt without class boundaries (the flat array's per-wave runs)
        auto emit_group = [&](const uint32_t *in, size_t n, int64_t &o, int64_t s0,
                              uint16_t *cum, uint32_t *dst, bool one_class = false) {
            auto cls_g = [&](uint32_t w) { return one_class ? 0 : cls_of(w); };
            std::fill(cls_cnt.begin(), cls_cnt.end(), 0);
            for (size_t i = 0; i < n; ++i) cls_cnt[cls_g(in[i])]++;
            uint32_t run = 0;
            for (int c = 0; c < 8; ++c) {
                cls_pos[c] = run;
                run += cls_cnt[c];
            }
            tmp.resize(n);
            for (size_t i = 0; i < n; ++i) tmp[cls_pos[cls_g(in[i])]++] = in[i];
            // The scorer's lanes take the group's postings in rounds from its start,
            // and a 32-lane group of its LDS updates is one set of 32 positions (by
            // 16-byte loads: p = 4 L + k of an aligned 128-block, one set per k; by
            // 4-byte loads: an aligned 32-block): each position takes, from its class,
            // a posting whose bank is not yet used in its set (bank cursor carried on
            // across sweeps and class boundaries), else any.
            uint32_t c0 = 0, usedq[4] = {0, 0, 0, 0};
            int cursor = 0;
            const int64_t o_start = o;
            for (int c = 0; c < 8; ++c) {
                const uint32_t c1 = c0 + cls_cnt[c];
                std::fill(bucket_cnt.begin(), bucket_cnt.end(), 0);
                for (uint32_t i = c0; i < c1; ++i) bucket_cnt[bank_of(tmp[i])]++;
                uint32_t r = 0, avail = 0;
                for (int k = 0; k < 32; ++k) {
                    head[k] = r;
                    r += bucket_cnt[k];
                    if (bucket_cnt[k]) avail |= 1u << k;
                }
                bk.resize(c1 - c0);
                fill = head;
                for (uint32_t i = c0; i < c1; ++i) bk[fill[bank_of(tmp[i])]++] = tmp[i];
                for (uint32_t i = c0; i < c1; ++i) {
                    const int64_t rp = o - o_start;
                    if ((rp & (deal_x4 ? 127 : 31)) == 0) usedq[0] = usedq[1] = usedq[2] = usedq[3] = 0;
                    uint32_t &used = usedq[deal_x4 ? (rp & 3) : 0];
                    uint32_t cand = avail & ~used;
                    if (!cand) cand = avail;  // every bank left is taken in this block
                    const uint32_t rot = cursor ? (cand >> cursor) | (cand << (32 - cursor)) : cand;
                    const int k = (__builtin_ctz(rot) + cursor) & 31;
                    dst[o++] = bk[head[k]++];
                    if (--bucket_cnt[k] == 0) avail &= ~(1u << k);
                    used |= 1u << k;
                    cursor = (k + 1) & 31;
                }
                if (cum) cum[c] = (uint16_t)(o - s0);
                c0 = c1;
            }
        };
        for (int64_t t = t0; t < t1; ++t) {
            for (uint32_t e = tb_start[t]; e < tb_start[t + 1]; ++e) {
                const int64_t s0 = epos[e], s1 = epos[e + 1];
                uint16_t *sg = &seg[(size_t)e * 8];
                grp.assign(packed.begin() + s0, packed.begin() + s1);
                uint32_t mx = 0;
                for (uint32_t x : grp) mx = std::max(mx, x & 255u);
                emax[e] = (uint8_t)mx;
                int64_t o = s0;
                const uint32_t id = lid[e];
                if (id == NO) {
                    emit_group(grp.data(), grp.size(), o, s0, sg, packed.data());
                    if (flat_runs)
                        std::copy(packed.begin() + s0, packed.begin() + o, flat.begin() + s0);
                    continue;
                }
                {  // whole-sublist class counts (seg), then the per-wave layout
                    uint32_t run = 0, cc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    for (uint32_t x : grp) cc[cls_of(x)]++;
                    for (int c = 0; c < 8; ++c) sg[c] = (uint16_t)(run += cc[c]);
                }
                for (int w = 0; w < WSEG; ++w) {
                    seg_in.clear();
                    uint32_t wm = 0;
                    for (uint32_t x : grp)
                        if (std::min<uint32_t>((x >> 8) / S, WSEG - 1) == (uint32_t)w) {
                            seg_in.push_back(x);
                            wm = std::max(wm, x & 255u);
                        }
                    wmax[(size_t)id * WSEG + w] = (uint8_t)wm;
                    const int64_t ow = o;
                    emit_group(seg_in.data(), seg_in.size(), o, s0,
                               &wmeta[(size_t)id * WSEG * 8 + w * 8], packed.data());
                    if (flat_runs) {
                        int64_t of = ow;
                        emit_group(seg_in.data(), seg_in.size(), of, s0, nullptr, flat.data(),
                                   true);
                    }
                }
            }
        }
    });
    for (auto &w : packed) w = (((w >> 8) << 10) | (w & 255u)) ^ POST_X;  // device encoding (see POST_X)
    for (auto &w : flat) w = (((w >> 8) << 10) | (w & 255u)) ^ POST_X;
    upload(ix->post, packed);
    if (flat_runs) upload(ix->post_flat, flat);
    ix->has_flat = flat_runs;
    upload(ix->tb_start, tb_start);
    upload(ix->eblk, eblk);
    upload(ix->epos, epos);
    upload(ix->seg, seg);
    upload(ix->lid, lid);
    upload(ix->wmeta, wmeta);
    upload(ix->emax, emax);
    upload(ix->wmax, wmax);
}

}  // namespace

static_assert(IL_BLOCK_DOCS == MAX_BLOCK_DOCS && IL_WSEG == WSEG && IL_WLONG_MIN == WLONG_MIN &&
                  IL_POST_X == POST_X,
              "index_layout.h builds the layout this scorer reads");

extern "C" {

// A di_index on `device` with its stream and the environment's settings, nothing built.
static std::unique_ptr<di_index> new_index(int device) {
    std::unique_ptr<di_index> ix(new di_index());
    ix->device = device;
    DI_HIP(hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking));
    ix->own_stream = true;
    if (const char *ab = std::getenv("DI_PROFILE_ABLATE")) ix->ablate = std::atoi(ab);
    if (const char *bo = std::getenv("DI_BLOCK_ORDER")) ix->block_order = bo[0] == '1';
    if (const char *st = std::getenv("DI_SCORE_THRESHOLD"))  // (tested both ways)
        ix->shared_thr = st[0] != '0' ? 1 : 0;
    if (const char *e = std::getenv("DI_TQ_EVERY")) ix->tq_every = std::max(1, std::atoi(e));
    if (const char *e = std::getenv("DI_TQ_FIRST")) ix->tq_first = std::max(0, std::atoi(e));
    return ix;
}

int di_index_create(const int64_t *term_off, int64_t n_terms, const uint32_t *pdoc,
                    const uint8_t *pval, uint32_t doc_lo, uint32_t doc_hi, int device,
                    di_index **out) {
    return guard([&] {
        DI_REQUIRE(out && term_off && (n_terms == 0 || (pdoc && pval)), DI_EINVAL,
                   "null argument");
        check_device(device);
        DeviceScope ds(device);
        std::unique_ptr<di_index> ix = new_index(device);
        build_index(ix.get(), term_off, n_terms, pdoc, pval, doc_lo, doc_hi);
        *out = ix.release();
    });
}

int di_index_create_device(const int64_t *term_off, int64_t n_terms, const uint32_t *pdoc,
                           const uint8_t *pval, uint32_t doc_lo, uint32_t doc_hi, int device,
                           void *hip_stream, uint32_t flags, di_index **out) {
    return guard([&] {
        DI_REQUIRE(out, DI_EINVAL, "null output");
        *out = nullptr;
        DI_REQUIRE(term_off && (n_terms == 0 || (pdoc && pval)), DI_EINVAL, "null argument");
        DI_REQUIRE(n_terms >= 0, DI_EINVAL, "n_terms < 0");
        DI_REQUIRE(n_terms < (int64_t)0xFFFFFFFF, DI_ERANGE, "n_terms %lld >= 2^32",
                   (long long)n_terms);
        check_device(device);
        DeviceScope ds(device);
        const bool dev = flags & DI_F_DEVICE_PTRS, timing = flags & DI_F_TIMING;
        hipStream_t s = (hipStream_t)hip_stream;
        std::unique_ptr<di_index> ix = new_index(device);
        DevBuf in_off, in_doc, in_val;
        size_t n_in = 0;  // postings a host caller's arrays hold: [0, term_off[n_terms])
        if (!dev) {       // (checked before anything is copied; the device checks again)
            DI_REQUIRE(term_off[0] >= 0, DI_EINVAL, "term_off[0] < 0");
            for (int64_t t = 0; t < n_terms; ++t)
                DI_REQUIRE(term_off[t + 1] >= term_off[t], DI_EINVAL,
                           "term_off not monotone at %lld", (long long)t);
            n_in = (size_t)term_off[n_terms];
        }
        const int64_t *d_off = stage_in(term_off, (size_t)n_terms + 1, dev, in_off, s);
        const uint32_t *d_doc = stage_in(pdoc, n_in, dev, in_doc, s);
        const uint8_t *d_val = stage_in(pval, n_in, dev, in_val, s);
        IndexLayout lay{&ix->post, &ix->post_flat, &ix->tb_start, &ix->eblk, &ix->epos,
                        &ix->seg,  &ix->lid,       &ix->wmeta,    &ix->emax, &ix->wmax};
        build_layout_device(d_off, n_terms, d_doc, d_val, doc_lo, doc_hi, s, timing, ix->timer,
                            lay);
        ix->n_terms = n_terms;
        ix->n_post = lay.n_post;
        ix->n_ent = lay.n_ent;
        ix->n_long = lay.n_long;
        ix->n_docs = lay.n_docs;
        ix->doc_lo = lay.doc_lo;
        ix->nb = lay.nb;
        ix->block_docs = lay.block_docs;
        ix->has_flat = lay.has_flat;
        *out = ix.release();
    });
}

int di_index_layout(const di_index *ix, int64_t *n_ent, int64_t *n_long, int32_t *block_docs,
                    int32_t *has_flat) {
    return guard([&] {
        DI_REQUIRE(ix, DI_EINVAL, "null handle");
        if (n_ent) *n_ent = ix->n_ent;
        if (n_long) *n_long = ix->n_long;
        if (block_docs) *block_docs = ix->block_docs;
        if (has_flat) *has_flat = ix->has_flat ? 1 : 0;
    });
}

int di_index_export(const di_index *ix, uint32_t *post, uint32_t *post_flat, uint32_t *tb_start,
                    uint16_t *eblk, uint32_t *epos, uint16_t *seg, uint32_t *lid, uint16_t *wmeta,
                    uint8_t *emax, uint8_t *wmax) {
    return guard([&] {
        DI_REQUIRE(ix, DI_EINVAL, "null handle");
        DI_REQUIRE(!post_flat || ix->has_flat, DI_EINVAL,
                   "no flat posting array (DI_DEAL_CLASSES=1 at create)");
        DeviceScope ds(ix->device);
        DI_HIP(hipStreamSynchronize(ix->stream));
        auto get = [](void *dst, const DevBuf &b, size_t bytes) {
            if (dst && bytes) DI_HIP(hipMemcpy(dst, b.p, bytes, hipMemcpyDeviceToHost));
        };
        const size_t np = (size_t)ix->n_post, ne = (size_t)ix->n_ent, nl = (size_t)ix->n_long;
        get(post, ix->post, np * 4);
        get(post_flat, ix->post_flat, np * 4);
        get(tb_start, ix->tb_start, ((size_t)ix->n_terms + 1) * 4);
        get(eblk, ix->eblk, ne * 2);
        get(epos, ix->epos, (ne + 1) * 4);
        get(seg, ix->seg, ne * 8 * 2);
        get(lid, ix->lid, ne * 4);
        get(wmeta, ix->wmeta, nl * WSEG * 8 * 2);
        get(emax, ix->emax, ne);
        get(wmax, ix->wmax, nl * WSEG);
    });
}

int di_index_load_reference(const char *dir, uint32_t doc_lo, uint32_t doc_hi, int device,
                            di_index **out) {
    return guard([&] {
        DI_REQUIRE(dir && out, DI_EINVAL, "null argument");
        std::string d(dir);
        // .idx read whole (16 B per term); .dat mapped: a doc-id shard reads only its
        // own postings out of it, on host_threads() threads (every rank of a sharded
        // rank CLI maps the same file: one page-cache copy, no per-rank whole-file copy)
        std::ifstream fi(d + "/inverted_index.idx", std::ios::binary | std::ios::ate);
        DI_REQUIRE(fi, DI_EIO, "cannot open %s/inverted_index.idx", dir);
        const size_t isz = (size_t)fi.tellg();
        DI_REQUIRE(isz % 16 == 0, DI_EFORMAT, "inverted_index.idx size %zu not a multiple of 16",
                   isz);
        std::vector<uint64_t> idx(isz / 8);
        fi.seekg(0);
        fi.read(reinterpret_cast<char *>(idx.data()), (std::streamsize)isz);
        DI_REQUIRE(fi || isz == 0, DI_EIO, "cannot read %s/inverted_index.idx", dir);
        const int fd = ::open((d + "/inverted_index.dat").c_str(), O_RDONLY);
        DI_REQUIRE(fd >= 0, DI_EIO, "cannot open %s/inverted_index.dat", dir);
        struct stat st;
        if (::fstat(fd, &st) != 0) {
            ::close(fd);
            DI_REQUIRE(false, DI_EIO, "cannot stat %s/inverted_index.dat", dir);
        }
        const size_t dsz = (size_t)st.st_size;
        const unsigned char *dat = nullptr;
        if (dsz) {
            void *m = ::mmap(nullptr, dsz, PROT_READ, MAP_SHARED, fd, 0);
            ::close(fd);
            DI_REQUIRE(m != MAP_FAILED, DI_EIO, "cannot map %s/inverted_index.dat", dir);
            dat = static_cast<const unsigned char *>(m);
        } else {
            ::close(fd);
        }
        struct Unmap {
            const void *p;
            size_t n;
            ~Unmap() {
                if (p) ::munmap(const_cast<void *>(p), n);
            }
        } unmap{dat, dsz};
        DI_REQUIRE(dsz % 5 == 0, DI_EFORMAT, "inverted_index.dat size %zu not a multiple of 5",
                   dsz);
        const int64_t nt = (int64_t)(isz / 16);
        for (int64_t t = 0; t < nt; ++t) {
            const uint64_t s = idx[2 * t], e = idx[2 * t + 1];
            DI_REQUIRE(s % 5 == 0 && e % 5 == 0 && s <= e && e <= dsz, DI_EFORMAT,
                       "bad (start,end) for term %lld", (long long)t);
        }
        const uint64_t hi = doc_hi ? doc_hi : 0x100000000ull;
        // postings of term t: records [start/5, end/5) up to its first 0 value
        // (create.py:45-51, inverted_index.py:50-51), docs of the shard only
        auto rec_doc = [&](uint64_t r) {
            uint32_t doc;
            std::memcpy(&doc, dat + r * 5, 4);
            return doc;
        };
        std::vector<int64_t> term_off((size_t)nt + 1, 0);
        parallel_for(nt, [&](int64_t t0, int64_t t1, int) {
            for (int64_t t = t0; t < t1; ++t) {
                int64_t c = 0;
                for (uint64_t r = idx[2 * t] / 5; r < idx[2 * t + 1] / 5; ++r) {
                    if (dat[r * 5 + 4] == 0) break;
                    const uint32_t doc = rec_doc(r);
                    c += doc >= doc_lo && doc < hi;
                }
                term_off[(size_t)t + 1] = c;
            }
        });
        for (int64_t t = 0; t < nt; ++t) term_off[(size_t)t + 1] += term_off[(size_t)t];
        const int64_t np = term_off[(size_t)nt];
        std::vector<uint32_t> pdoc((size_t)std::max<int64_t>(np, 1));
        std::vector<uint8_t> pval((size_t)std::max<int64_t>(np, 1));
        parallel_for(nt, [&](int64_t t0, int64_t t1, int) {
            for (int64_t t = t0; t < t1; ++t) {
                int64_t o = term_off[(size_t)t];
                for (uint64_t r = idx[2 * t] / 5; r < idx[2 * t + 1] / 5; ++r) {
                    const uint8_t v = dat[r * 5 + 4];
                    if (v == 0) break;
                    const uint32_t doc = rec_doc(r);
                    if (doc >= doc_lo && doc < hi) {
                        pdoc[(size_t)o] = doc;
                        pval[(size_t)o++] = v;
                    }
                }
            }
        });
        // the parsed CSR goes to the device layout builder (its median time is below the
        // host route's fastest at 100 k, 1.1 M and 8.8 M docs);
        // DI_INDEX_LAYOUT=host: build_index() on host threads, the same bytes
        const char *lay = std::getenv("DI_INDEX_LAYOUT");
        const int rc = !(lay && std::strcmp(lay, "host") == 0)
                           ? di_index_create_device(term_off.data(), nt, pdoc.data(), pval.data(),
                                                    doc_lo, doc_hi, device, nullptr, 0, out)
                           : di_index_create(term_off.data(), nt, pdoc.data(), pval.data(), doc_lo,
                                             doc_hi, device, out);
        if (rc != DI_OK) throw Error{rc};
    });
}

int di_index_reserve(di_index *ix, int32_t max_q, int32_t k) {
    return guard([&] {
        DI_REQUIRE(ix && max_q >= 0 && k > 0 && k <= DI_MAX_TOPK, DI_EINVAL, "bad argument");
        DeviceScope ds(ix->device);
        // (the few-block emit-above selection lists up to 2 k keys per item, see search)
        const int kl = ix->list_cap(k);
        size_t nbk = (size_t)max_q * std::max(ix->nb, 1) * kl;
        ix->ws_ck.reserve(nbk * 8);
        ix->ws_cn.reserve((size_t)max_q * std::max(ix->nb, 1) * 4);
    });
}

int di_index_search(di_index *ix, const uint32_t *q_terms, const int32_t *cu_q, int32_t n_q,
                    int32_t k, uint32_t *out_doc, uint32_t *out_score, int32_t *out_n,
                    uint64_t *out_key, uint32_t flags) {
    return guard([&] {
        DI_REQUIRE(ix && cu_q && out_doc && out_score && out_n, DI_EINVAL, "null argument");
        DI_REQUIRE(n_q >= 0, DI_EINVAL, "n_q < 0");
        DI_REQUIRE(k > 0 && k <= DI_MAX_TOPK, DI_ERANGE, "k=%d outside [1, %d]", k,
                   DI_MAX_TOPK);
        DeviceScope ds(ix->device);
        const bool dev = flags & DI_F_DEVICE_PTRS;
        const bool timing = flags & DI_F_TIMING;
        hipStream_t s = ix->stream;
        if (n_q == 0) return;
        int64_t nterms_total = 0;
        int max_nt = WTERMS;  // record slots per item (device pointers: the per-wave maximum)
        if (!dev) {
            max_nt = 1;
            for (int q = 0; q < n_q; ++q) {
                int32_t c = cu_q[q + 1] - cu_q[q];
                max_nt = std::max(max_nt, (int)c);
                DI_REQUIRE(c >= 0, DI_EINVAL, "cu_q not monotone at %d", q);
                DI_REQUIRE(c <= DI_MAX_QUERY_TERMS, DI_ERANGE,
                           "query %d has %d terms (limit %d)", q, c, DI_MAX_QUERY_TERMS);
                DI_REQUIRE(c <= DI_SHORT_QUERY_TERMS ||
                               (uint64_t)ix->doc_lo + ix->n_docs <= (1ull << 24),
                           DI_ERANGE,
                           "query %d has %d terms: queries over %d terms need shard docs < 2^24",
                           q, c, DI_SHORT_QUERY_TERMS);
            }
            nterms_total = cu_q[n_q];
            for (int64_t i = 0; i < nterms_total; ++i)
                DI_REQUIRE(q_terms[i] < (uint64_t)ix->n_terms, DI_EINVAL,
                           "term id %u out of range", q_terms[i]);
        }
        const int nb = std::max(ix->nb, 1);
        // query chunking keeps the candidate workspace bounded: 4 GiB of the 288 GB HBM
        // (DI_CAND_WS_MIB overrides, A/B).  A 1 GiB cap cut 8.8 M-doc batches into 14
        // chunks of 499 queries, whose merge launches had ~2 workgroups per CU
        // (round-4 DESIGN §4).
        // The item records (item_setup_kernel) take rec_slots per item -- the batch's
        // longest query up to WTERMS (~6 for MS MARCO queries, 64 with device-pointer
        // queries) -- and are capped at twice the candidate cap, which bounds the chunk
        // too: one setting (DI_CAND_WS_MIB) sizes both.  Peak workspace of a handle
        // ~3x the cap.
        const int rec_slots = std::min(std::max(max_nt, 1), WTERMS);
        // Few blocks: the emit-above selection (di_index::few_blocks)
        const bool few = ix->few_blocks(k);
        const int kl = ix->list_cap(k);
        const int64_t per_q = (int64_t)nb * kl * 8;
        const int64_t rec_per_q = (int64_t)nb * rec_slots * (int64_t)sizeof(ItemRec);
        int64_t ws_cap = 4ll << 30;
        if (const char *e = std::getenv("DI_CAND_WS_MIB")) ws_cap = std::max(1ll, std::atoll(e)) << 20;
        const int chunk = (int)std::max<int64_t>(
            1, std::min<int64_t>({(int64_t)n_q, ws_cap / per_q, 2 * ws_cap / rec_per_q}));
        ix->ws_ck.reserve((size_t)chunk * per_q);
        ix->ws_cn.reserve((size_t)chunk * nb * 4);
        ix->ws_thr.reserve((size_t)chunk * QH_BINS * 4);
        ix->ws_long.reserve(4);
        if (!ix->bm_stat.p) {
            ix->bm_stat.reserve(16);
            DI_HIP(hipMemsetAsync(ix->bm_stat.p, 0, 16, s));
        }
        // (AB_NO_RECORDS: the scorer walks the chain itself, A/B and the fallback test)
        const size_t rec_bytes = (size_t)chunk * rec_per_q;
        const bool use_rec = !(ix->ablate & AB_NO_RECORDS);
        if (use_rec) ix->ws_rec.reserve(rec_bytes);
        const uint32_t *dq = stage_in(q_terms, (size_t)nterms_total, dev, ix->ws_q, s);
        const int32_t *dcu = stage_in(cu_q, (size_t)n_q + 1, dev, ix->ws_cu, s);
        const size_t nk = (size_t)n_q * k;
        StagedOut<uint32_t> doc(out_doc, nk, dev, ix->ws_doc), score(out_score, nk, dev, ix->ws_score);
        StagedOut<int32_t> on(out_n, (size_t)n_q, dev, ix->ws_n);
        StagedOut<uint64_t> key(out_key, nk, dev, ix->ws_key);
        for (int q0 = 0; q0 < n_q; q0 += chunk) {
            const int nq = std::min(chunk, n_q - q0);
            if (ix->nb == 0) {
                DI_HIP(hipMemsetAsync(ix->ws_cn.p, 0, (size_t)nq * nb * 4, s));
            } else {
                const bool thr = nb > 1 && (ix->shared_thr < 0 ? nb >= 8 : ix->shared_thr == 1);
                if (thr) DI_HIP(hipMemsetAsync(ix->ws_thr.p, 0, (size_t)nq * QH_BINS * 4, s));
                DI_HIP(hipMemsetAsync(ix->ws_long.p, 0, 4, s));
                TimedLaunch tl(ix->timer, timing, "score_blocks", s);  // (both kernels)
                const int n_items = nq * nb;
                // packed postings (configs[4]): exact scoring from the item records only
                // (records always fit: the chunk is bounded by them; AB_NO_RECORDS turns
                // them off, and the packed layout with them)
                const bool pk = ix->packed && ix->pk_built && ix->min_cls >= 7 && use_rec;
                // block-max: blocks in descending order of their bound per query, opt-in
                // (DI_BLOCK_ORDER=1): it raises the running threshold sooner but gives up
                // the block-major L2 sharing of the popular sublists -- at 8.8 M docs, f = 1:
                // skewed 79.4 vs 76.7 ms per batch, i.i.d. 126.0 vs 114.2 (round-4 DESIGN §4)
                const bool order = thr && ix->bm_factor > 0.0f && nb > 1 &&
                                   nb <= BO_MAX_BLOCKS && ix->block_order;
                if (order) ix->ws_border.reserve((size_t)nq * nb * 2);
                // (AB_HIST_THRESHOLD: the histogram-copy threshold instead, A/B)
                // (DI_TQ_EVERY / DI_TQ_FIRST: the threshold refresh schedule of score_item;
                // every = 1: every item copies the histogram, as before round 6)
                const bool sched = thr && ix->tq_every > 1;
                const bool use_qtq =
                    (thr && ix->bm_factor > 0.0f && !(ix->ablate & AB_HIST_THRESHOLD)) || few || sched;
                if (use_qtq) {
                    ix->ws_tq.reserve((size_t)nq * 4);
                    DI_HIP(hipMemsetAsync(ix->ws_tq.p, 0, (size_t)nq * 4, s));
                }
                ScoreLaunch L{};
                ScoreArgs &a = L.a;
                a.post = ix->post_for(ix->min_cls);
                a.si = ix->sub(pk);
                a.min_cls = ix->min_cls, a.nb = nb, a.block_docs = ix->block_docs;
                a.n_terms = ix->n_terms, a.n_docs = ix->n_docs, a.doc_lo = ix->doc_lo;
                a.q_terms = dq, a.cu_q = dcu + q0;
                a.k = k, a.kl = kl;
                a.cand_key = ix->ws_ck.as<uint64_t>(), a.cand_n = ix->ws_cn.as<int32_t>();
                a.n_items = n_items, a.n_q = nq;
                a.qhist = thr ? ix->ws_thr.as<uint32_t>() : nullptr;
                a.ablate = ix->ablate;
                a.rec = use_rec ? ix->ws_rec.as<ItemRec>() : nullptr, a.rec_slots = rec_slots;
                a.long_flag = ix->ws_long.as<uint32_t>();
                a.bm_factor = thr ? ix->bm_factor : 0.0f;
                a.bm_stat = ix->bm_stat.as<unsigned long long>();
                a.border = order ? ix->ws_border.as<uint16_t>() : nullptr;
                a.qtq = use_qtq ? ix->ws_tq.as<uint32_t>() : nullptr;
                a.tq_sched = sched ? (ix->tq_first << 16) | ix->tq_every : 1;
                // (AB_FORCE_EXT_BM: the block-max instantiation with block-max off, A/B of
                // its code alone)
                // Heavily pruned searches (min_impact >= 16: min_cls <= 3) run the EXT_BM
                // instantiation too, block-max off, for its one-sweep selection of sparse
                // items (score_item).  8.8 M docs, k q/s: skewed m 16 / 32 / 64 / 128
                // 110.8 / 96.9 / 98.2 / 98.6 -> 121.4 / 124.9 / 131.2 / 133.1; i.i.d. 2.5-4%
                // slower (the instantiation's own cost, items there rarely sparse); lighter
                // pruning 1-4% slower, so it keeps the plain kernel (round-4 DESIGN §4).
                L.pk = pk;
                L.ext = pk || order || (thr && ix->bm_factor > 0.0f) ||
                        (thr && ix->min_cls <= 3) || (ix->ablate & AB_FORCE_EXT_BM);
                L.few = few;
                L.stream = s;
                launch_score(L);
            }
            {
                TimedLaunch tl(ix->timer, timing, "merge_topk", s);
                launch_merge(ix->ws_ck.as<uint64_t>(), ix->ws_cn.as<int32_t>(), nq, nb, kl, k,
                             key.d ? key.d + (int64_t)q0 * k : nullptr, doc.d + (int64_t)q0 * k,
                             score.d + (int64_t)q0 * k, on.d + q0, DECODE_QUANT, s, false,
                             dcu + q0);
            }
        }
        doc.copy_back(s);
        score.copy_back(s);
        on.copy_back(s);
        key.copy_back(s);
        if (!(flags & DI_F_ASYNC) || !dev) {
            DI_HIP(hipStreamSynchronize(s));
            ix->timer.resolve();
            if (!dev)
                for (int q = 0; q < n_q; ++q)
                    DI_REQUIRE(out_n[q] >= 0, DI_ERANGE, "query %d exceeded a kernel limit", q);
        }
    });
}

int di_index_info(const di_index *ix, int64_t *n_terms, int64_t *n_postings, uint32_t *n_docs,
                  int32_t *n_blocks) {
    return guard([&] {
        DI_REQUIRE(ix, DI_EINVAL, "null handle");
        if (n_terms) *n_terms = ix->n_terms;
        if (n_postings) *n_postings = ix->n_post;
        if (n_docs) *n_docs = ix->n_docs;
        if (n_blocks) *n_blocks = ix->nb;
    });
}

int di_index_set_min_impact(di_index *ix, int32_t min_impact) {
    return guard([&] {
        DI_REQUIRE(ix, DI_EINVAL, "null handle");
        DI_REQUIRE(min_impact >= 1 && min_impact <= 255, DI_ERANGE,
                   "min_impact=%d outside [1, 255]", min_impact);
        // postings with value >= 2^floor(log2 min_impact): the class prefix
        ix->min_cls = 7 - (31 - __builtin_clz((unsigned)min_impact));
    });
}

int di_index_set_block_max(di_index *ix, float factor) {
    return guard([&] {
        DI_REQUIRE(ix, DI_EINVAL, "null handle");
        DI_REQUIRE(factor == 0.0f || (factor >= 1.0f && factor <= 16.0f), DI_ERANGE,
                   "block-max factor %g: 0 (off) or in [1, 16]", (double)factor);
        ix->bm_factor = factor;
    });
}

// Packed (block-compressed) postings from the device layout: every run (short
// sublist, or one wave segment's run of a long one) sorted by doc, cut into frames of
// up to PK_FRAME postings, each frame bit-packed with its own widths (see
// packed_fields).  Host threads over entry ranges; three passes (frame counts, widths,
// encoding) so every entry writes its own ranges.
static void build_packed(di_index *ix) {
    const int64_t ne = ix->n_ent, np = ix->n_post, nl = ix->n_long;
    std::vector<uint32_t> post((size_t)std::max<int64_t>(np, 1)), epos((size_t)ne + 1);
    std::vector<uint32_t> lid((size_t)std::max<int64_t>(ne, 1));
    std::vector<uint16_t> wmeta((size_t)std::max<int64_t>(nl, 1) * WSEG * 8);
    if (np) DI_HIP(hipMemcpy(post.data(), ix->post.p, (size_t)np * 4, hipMemcpyDeviceToHost));
    DI_HIP(hipMemcpy(epos.data(), ix->epos.p, ((size_t)ne + 1) * 4, hipMemcpyDeviceToHost));
    if (ne) DI_HIP(hipMemcpy(lid.data(), ix->lid.p, (size_t)ne * 4, hipMemcpyDeviceToHost));
    if (nl)
        DI_HIP(hipMemcpy(wmeta.data(), ix->wmeta.p, (size_t)nl * WSEG * 8 * 2,
                         hipMemcpyDeviceToHost));
    const uint32_t NO = 0xFFFFFFFFu;
    // run r of entry e: [a, b) of the postings (w: segment of a long entry)
    auto run_of = [&](int64_t e, int w, uint32_t &a, uint32_t &b) {
        const uint32_t id = lid[(size_t)e];
        if (id == NO) {
            a = epos[(size_t)e];
            b = epos[(size_t)e + 1];
            return;
        }
        const uint16_t *m = &wmeta[(size_t)id * WSEG * 8];
        a = epos[(size_t)e] + (w ? m[(w - 1) * 8 + 7] : 0u);
        b = epos[(size_t)e] + m[w * 8 + 7];
    };
    // (a short sublist under PK_MIN postings stays plain: no run, no frame)
    auto n_runs = [&](int64_t e) {
        return lid[(size_t)e] != NO ? WSEG : epos[(size_t)e + 1] - epos[(size_t)e] >= PK_MIN ? 1 : 0;
    };
    auto frames_of = [](uint32_t n) { return (n + PK_FRAME - 1) / PK_FRAME; };
    // pass 1: frames per entry -> fs; per long entry the run starts (fwt)
    std::vector<uint32_t> fs((size_t)ne + 1, 0);
    std::vector<uint16_t> fwt((size_t)std::max<int64_t>(nl, 1) * (WSEG + 1), 0);
    parallel_for(ne, [&](int64_t e0, int64_t e1, int) {
        for (int64_t e = e0; e < e1; ++e) {
            uint32_t nf = 0;
            const uint32_t id = lid[(size_t)e];
            for (int w = 0; w < n_runs(e); ++w) {
                uint32_t a, b;
                run_of(e, w, a, b);
                if (id != NO) fwt[(size_t)id * (WSEG + 1) + w] = (uint16_t)nf;
                nf += frames_of(b - a);
            }
            if (id != NO) fwt[(size_t)id * (WSEG + 1) + WSEG] = (uint16_t)nf;
            fs[(size_t)e + 1] = nf;
        }
    });
    for (int64_t e = 0; e < ne; ++e) fs[(size_t)e + 1] += fs[(size_t)e];
    const int64_t nfr = fs[(size_t)ne];
    // one run's frames: sorted (doc, value), per frame (bd, bv, vmin, W)
    struct FrameInfo {
        uint32_t base, cnt, bd, bv, vmin, W;
    };
    auto bits = [](uint32_t x) { return x ? 32 - __builtin_clz(x) : 0; };
    auto frame_info = [&](const std::vector<std::pair<uint32_t, uint32_t>> &dv, size_t i0,
                          size_t i1) {
        FrameInfo fi{dv[i0].first, (uint32_t)(i1 - i0), 0, 0, 255, 0};
        uint32_t dmax = 0, vmax = 0;
        for (size_t i = i0; i < i1; ++i) {
            if (i > i0) dmax = std::max(dmax, dv[i].first - dv[i - 1].first);
            fi.vmin = std::min(fi.vmin, dv[i].second);
            vmax = std::max(vmax, dv[i].second);
        }
        fi.bd = (uint32_t)bits(dmax);
        fi.bv = (uint32_t)bits(vmax - fi.vmin);
        fi.W = std::max<uint32_t>(4, (fi.bd + fi.bv + 3) / 4 * 4);
        return fi;
    };
    auto sorted_run = [&](uint32_t a, uint32_t b, std::vector<std::pair<uint32_t, uint32_t>> &dv) {
        dv.resize(b - a);
        for (uint32_t p = a; p < b; ++p)
            dv[p - a] = {(post[p] ^ POST_X) >> 10, post[p] & 255u};
        std::sort(dv.begin(), dv.end());
    };
    // pass 2: data dwords per frame
    std::vector<uint32_t> fdw((size_t)std::max<int64_t>(nfr, 1) + 1, 0);
    parallel_for(ne, [&](int64_t e0, int64_t e1, int) {
        std::vector<std::pair<uint32_t, uint32_t>> dv;
        for (int64_t e = e0; e < e1; ++e) {
            uint32_t f = fs[(size_t)e];
            for (int w = 0; w < n_runs(e); ++w) {
                uint32_t a, b;
                run_of(e, w, a, b);
                sorted_run(a, b, dv);
                for (size_t i0 = 0; i0 < dv.size(); i0 += PK_FRAME, ++f) {
                    const size_t i1 = std::min(dv.size(), i0 + PK_FRAME);
                    const FrameInfo fi = frame_info(dv, i0, i1);
                    fdw[(size_t)f + 1] = (uint32_t)((fi.cnt + PK_PER_LANE - 1) / PK_PER_LANE) * (fi.W / 4);
                }
            }
        }
    });
    std::vector<uint64_t> doff((size_t)nfr + 1, 0);
    for (int64_t f = 0; f < nfr; ++f) doff[(size_t)f + 1] = doff[(size_t)f] + fdw[(size_t)f + 1];
    DI_REQUIRE(doff[(size_t)nfr] < 0xFFFFFFFFull, DI_ERANGE, "packed postings past 2^32 dwords");
    // pass 3: headers and data
    std::vector<uint4> fh((size_t)std::max<int64_t>(nfr, 1));
    std::vector<uint32_t> data((size_t)std::max<uint64_t>(doff[(size_t)nfr], 1), 0);
    parallel_for(ne, [&](int64_t e0, int64_t e1, int) {
        std::vector<std::pair<uint32_t, uint32_t>> dv;
        for (int64_t e = e0; e < e1; ++e) {
            uint32_t f = fs[(size_t)e];
            for (int w = 0; w < n_runs(e); ++w) {
                uint32_t a, b;
                run_of(e, w, a, b);
                sorted_run(a, b, dv);
                for (size_t i0 = 0; i0 < dv.size(); i0 += PK_FRAME, ++f) {
                    const size_t i1 = std::min(dv.size(), i0 + PK_FRAME);
                    const FrameInfo fi = frame_info(dv, i0, i1);
                    uint32_t *out = &data[(size_t)doff[(size_t)f]];
                    const uint32_t nd = fi.W / 4;
                    for (size_t i = i0; i < i1; ++i) {
                        const uint32_t k = (uint32_t)(i - i0);
                        const uint32_t delta = i > i0 ? dv[i].first - dv[i - 1].first : 0u;
                        const uint64_t field = (uint64_t)delta | ((uint64_t)(dv[i].second - fi.vmin) << fi.bd);
                        const uint32_t lane = k / PK_PER_LANE, slot = k % PK_PER_LANE;
                        const uint64_t bit = (uint64_t)lane * nd * 32 + (uint64_t)slot * fi.W;
                        const uint64_t sh = field << (bit & 31);
                        out[bit >> 5] |= (uint32_t)sh;
                        if ((bit & 31) + fi.W > 32) out[(bit >> 5) + 1] |= (uint32_t)(sh >> 32);
                    }
                    fh[(size_t)f] = make_uint4((uint32_t)doff[(size_t)f],
                                               fi.base | (fi.cnt << 16) | (fi.bd << 26),
                                               fi.vmin | (fi.bv << 8) | (fi.W << 12), 0u);
                }
            }
        }
    });
    upload(ix->pk_fs, fs);
    upload(ix->pk_fwt, fwt);
    upload(ix->pk_fh, fh);
    upload(ix->pk_data, data);
    ix->pk_frames = nfr;
    // bytes the packed scorer reads: headers + packed data + the plain words of the short
    // sublists it reads from the plain layout
    int64_t plain_small = 0;
    for (int64_t e = 0; e < ne; ++e)
        if (n_runs(e) == 0) plain_small += epos[(size_t)e + 1] - epos[(size_t)e];
    ix->pk_bytes = (int64_t)doff[(size_t)nfr] * 4 + nfr * (int64_t)sizeof(uint4) + 4 * plain_small;
    ix->pk_built = true;
}

int di_index_set_packed(di_index *ix, int32_t on, int64_t *packed_bytes) {
    return guard([&] {
        DI_REQUIRE(ix, DI_EINVAL, "null handle");
        DeviceScope ds(ix->device);
        if (on && !ix->pk_built) {
            DI_HIP(hipStreamSynchronize(ix->stream));
            build_packed(ix);
        }
        ix->packed = on != 0;
        if (packed_bytes) *packed_bytes = ix->pk_built ? ix->pk_bytes : 0;
    });
}

int di_index_set_stream(di_index *ix, void *stream) {
    return guard([&] {
        DI_REQUIRE(ix, DI_EINVAL, "null handle");
        DeviceScope ds(ix->device);
        if (ix->own_stream && ix->stream) DI_HIP(hipStreamDestroy(ix->stream));
        ix->own_stream = stream == nullptr;
        if (stream)
            ix->stream = (hipStream_t)stream;
        else
            DI_HIP(hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking));
    });
}

int di_index_sync(di_index *ix) {
    return guard([&] {
        DI_REQUIRE(ix, DI_EINVAL, "null handle");
        DeviceScope ds(ix->device);
        DI_HIP(hipStreamSynchronize(ix->stream));
        ix->timer.resolve();
    });
}

int di_index_timing(di_index *ix, const char *name, di_timing *out, int reset) {
    return guard([&] {
        DI_REQUIRE(ix && name && out, DI_EINVAL, "null argument");
        const std::string n(name);
        if (n == "bm_segments" || n == "bm_segments_skipped") {
            // block-max counters (launches = the count; ms = 0), accumulated on the device
            // since the last reset: reading them synchronises the index's stream
            DeviceScope ds(ix->device);
            unsigned long long st[2] = {0, 0};
            if (ix->bm_stat.p) {
                read_back(st, ix->bm_stat.p, ix->stream);
                if (reset) DI_HIP(hipMemset(ix->bm_stat.p, 0, 16));
            }
            out->ms = 0.0;
            out->launches = (int64_t)st[n == "bm_segments" ? 0 : 1];
            return;
        }
        ix->timer.get(name, out, reset != 0);
    });
}

int di_index_destroy(di_index *ix) {
    return guard([&] {
        if (!ix) return;
        {
            DeviceScope ds(ix->device);
            if (ix->own_stream && ix->stream) (void)hipStreamDestroy(ix->stream);
        }
        delete ix;
    });
}

}  // extern "C"
