// Stateful cursor API: TraversalEngine.seek / next / previous / hasNext / hasPrevious
// (J/utils/traversal/TraversalEngine.java:241-339).  The state lives in HBM; each call is a
// one-thread kernel that reuses the device primitives of the batched walk (engine.h), so the cursor
// and the walk cannot drift apart.
#include "cursor.h"
#include "wavescan.h"

namespace ldbg {

template <int W>
struct CursorStateDev {
    Node cur;
    Node nxt, prv;
    uint32_t has_next, has_prev, first, go_forward, status;
    LsSaved ls;
    uint32_t vt_used, nxt_words_valid;
    uint64_t cur_words[W];     // k-mer of the cursor vertex (vertices without a record have no row to read it from)
    // outputs of the last step
    uint64_t out_words[W];
    int64_t out_rec;
};

// POOLED (a slot of the batch pool, below): the table is not cleared; a fresh `seen` is a new epoch, which the caller has chosen, and
// st.vt_used goes on counting the slots claimed since the table was last swept
template <int W, bool POOLED = false>
LDBG_DEV void cs_reseek(const EngineView& e, CursorStateDev<W>& st, uint64_t* vtab, uint32_t vcap) {
    // seek(sk) :321-335 — unique neighbours, fresh LinkStore, fresh `seen`
    if (!POOLED && st.vt_used != 0) for (uint32_t i = 0; i < vcap; i++) vtab[i] = 0;    // seen = new HashSet<>()
    VisitedTable vt;
    vt.tab = vtab; vt.mask = vcap - 1; vt.used = POOLED ? st.vt_used : 0;
    node_locate(vt, st.cur);
    st.has_next = popc4(st.cur.next_mask) == 1;
    if (st.has_next) { node_child_located(e, vt, st.cur, true, lowbit4(st.cur.next_mask), st.nxt); st.nxt_words_valid = 0; }
    st.has_prev = popc4(st.cur.prev_mask) == 1;
    if (st.has_prev) { node_child_located(e, vt, st.cur, false, lowbit4(st.cur.prev_mask), st.prv); }
    st.ls = LsSaved{};
    st.first = 1;
    st.vt_used = vt.used;
    st.status = st.cur.npe ? (uint32_t)ST_NULLPTR : (uint32_t)ST_OK;
}

template <int W>
LDBG_KERNEL void k_cursor_seek(EngineView e, CursorStateDev<W>* stp, const uint64_t* words, int is_kmer, uint64_t* vtab, uint32_t vcap) {
    if (global_tid() != 0) return;
    CursorStateDev<W>& st = *stp;
    Kmer<W> sk;
    for (int i = 0; i < W; i++) sk.w[i] = words[i];
    if (is_kmer) node_find<W>(e, sk, st.cur);
    else node_null(e, st.cur);
    for (int i = 0; i < W; i++) st.cur_words[i] = sk.w[i];
    cs_reseek<W>(e, st, vtab, vcap);
}

// one next() / previous() on the device-resident state
// (POOLED: `epoch` is the slot's current generation of `seen`; nothing is marked between a seek and the first step's re-seek, so that
// re-seek keeps the epoch.  The slot's start rule bounds the table's load, cursor_batch_item.)
template <int W, bool POOLED = false>
LDBG_DEV void cs_step(const EngineView& e, CursorStateDev<W>& st, bool fwd, uint64_t* vtab, uint32_t vcap, LsElem* els, uint32_t ecap, uint32_t epoch = 1) {
    st.status = ST_OK;
    if (st.first || (st.go_forward != 0) != fwd) {      // :243-248 / :283-288
        st.go_forward = fwd ? 1 : 0;
        cs_reseek<W, POOLED>(e, st, vtab, vcap);
        if (st.status != ST_OK) return;
    }
    VisitedTable vt;
    vt.tab = vtab; vt.mask = vcap - 1; vt.used = st.vt_used;
    if (!POOLED && vt.used * 2 > vcap) { st.status = ST_POOL_FULL; return; }   // more steps since seek() than the cursor's `seen` table holds
    // the nodes were saved by an earlier launch: bring their cached table entries up to date
    node_locate(vt, st.cur);
    if (st.has_next) node_locate(vt, st.nxt);
    if (st.has_prev) node_locate(vt, st.prv);
    vt.used = st.vt_used;
    LinkStoreDev ls;
    ls.fast = nullptr; ls.fast_cap = 0; ls.fast_stride = 0;
#ifdef LDBG_WALK_DIAG
    ls.diag = nullptr;
#endif
    ls.el = els; ls.cap = ecap;
    ls_restore(ls, st.ls);
    ls.overflow = false;
    Cursor cu;
    cu.cur = st.cur; cu.first = st.first != 0; cu.status = ST_OK; cu.epoch = epoch;
    cu.has = fwd ? st.has_next != 0 : st.has_prev != 0;
    if (!cu.has) { st.status = ST_NULLPTR; return; }   // target vanished after the re-seek: NPE in the reference
    cu.nxt = fwd ? st.nxt : st.prv;
    Node old = st.cur;
    // k-mer of the vertex stepped onto: from its row, or (no record) from the cursor k-mer and the edge base
    Kmer<W> tk;
    if (cu.nxt.idx >= 0) tk = node_kmer<W>(e, cu.nxt);
    else if (old.idx >= 0) tk = child_kmer<W>(e, old, fwd, cu.nxt.base);
    else { for (int i = 0; i < W; i++) tk.w[i] = st.cur_words[i]; }
    Node t = cursor_step<W>(e, cu, ls, vt, fwd);
    st.first = 0;
    st.cur = cu.cur;
    if (fwd) { st.prv = old; st.has_prev = 1; st.nxt = cu.nxt; st.has_next = cu.has ? 1 : 0; }
    else { st.nxt = old; st.has_next = 1; st.prv = cu.nxt; st.has_prev = cu.has ? 1 : 0; }
    st.ls = ls_save(ls);
    st.status = cu.status;
    st.vt_used = vt.used;
    for (int i = 0; i < W; i++) { st.out_words[i] = tk.w[i]; st.cur_words[i] = tk.w[i]; }
    st.out_rec = t.idx;
}
template <int W>
LDBG_KERNEL void k_cursor_step(EngineView e, CursorStateDev<W>* stp, int fwd_i, uint64_t* vtab, uint32_t vcap, LsElem* els, uint32_t ecap) {
    if (global_tid() != 0) return;
    cs_step<W>(e, *stp, fwd_i != 0, vtab, vcap, els, ecap);
}
// assemble(seed, goForward) (TraversalEngine.java:125-145) after a seek(seed): next() / previous() for as long as the cursor has one and
// fewer than max_len vertices have been collected, all in ONE launch; out_n[0] = vertices, out_n[1] = status of the last step
template <int W>
LDBG_KERNEL void k_cursor_assemble(EngineView e, CursorStateDev<W>* stp, int fwd_i, uint64_t* vtab, uint32_t vcap, LsElem* els, uint32_t ecap, int64_t max_len,
                                   uint64_t* out_words, int64_t* out_rec, int64_t* out_n) {
    if (global_tid() != 0) return;
    CursorStateDev<W>& st = *stp;
    const bool fwd = fwd_i != 0;
    int64_t n = 0;
    uint32_t status = st.status;
    while (status == ST_OK && (fwd ? st.has_next : st.has_prev) && n < max_len) {
        cs_step<W>(e, st, fwd, vtab, vcap, els, ecap);
        status = st.status;
        if (status != ST_OK) break;
        for (int i = 0; i < W; i++) out_words[n * W + i] = st.out_words[i];
        out_rec[n] = st.out_rec;
        n++;
    }
    out_n[0] = n; out_n[1] = (int64_t)status;
}

// ------------------------------------------------------------------ host
struct CursorHost::Impl {
    void* d_state = nullptr;
    void* d_vtab = nullptr;
    void* d_ls = nullptr;
    void* d_words = nullptr;
    uint32_t vcap = 1u << 17, ecap = 256;
    size_t state_bytes = 0;
    bool sought = false;
};

CursorHost::CursorHost(Engine& e) : eng_(e), impl_(new Impl) {
    e.enter();
    const int W = e.graph->hdr.W;
    impl_->state_bytes = with_words(W, [](auto w_) { return sizeof(CursorStateDev<decltype(w_)::value>); });
    impl_->d_state = rt::dmalloc(impl_->state_bytes);
    impl_->d_vtab = rt::dmalloc((size_t)impl_->vcap * 8);
    impl_->d_ls = rt::dmalloc((size_t)impl_->ecap * sizeof(LsElem));
    impl_->d_words = rt::dmalloc((size_t)W * 8);
    rt::dmemset(impl_->d_state, 0, impl_->state_bytes, e.estream());
    rt::dmemset(impl_->d_vtab, 0, (size_t)impl_->vcap * 8, e.estream());
    rt::stream_sync(e.estream());
}
CursorHost::~CursorHost() {
    rt::dfree(impl_->d_state); rt::dfree(impl_->d_vtab); rt::dfree(impl_->d_ls); rt::dfree(impl_->d_words);
    delete impl_;
}

template <int W>
static void read_state(void* d, CursorStateDev<W>& h, rt::stream_t s) {
    rt::d2h(&h, d, sizeof(h), s);
    rt::stream_sync(s);
}

void CursorHost::check_status(uint32_t st) {
    if (st == ST_NULLPTR) throw StatusError(LDBG_ERR_NULLPOINTER, "cursor dereferenced a missing record / vanished target (NullPointerException in the reference)");
    if (st == ST_LINKSTORE_FULL) throw StatusError(LDBG_ERR_CAPACITY, "cursor link store capacity exceeded");
    if (st == ST_POOL_FULL) throw StatusError(LDBG_ERR_CAPACITY, "cursor walked more than 65536 steps since the last seek()");
}

void CursorHost::seek(const char* kmer) {
    eng_.enter();
    const int W = eng_.graph->hdr.W, k = eng_.graph->hdr.k;
    rt::stream_t s = eng_.estream();
    std::vector<uint64_t> w(W);
    const int is_kmer = ascii_to_words(kmer, k, w.data(), W) ? 1 : 0;       // validity beside the words: at k = 32, 64, ... no bit pattern is free (Q4)
    if (!is_kmer) std::fill(w.begin(), w.end(), 0ull);
    rt::h2d(impl_->d_words, w.data(), (size_t)W * 8, s);
    with_words(W, [&](auto w_) {
        constexpr int WW = decltype(w_)::value;
        LDBG_LAUNCH(k_cursor_seek<WW>, 1, 64, s, eng_.view, (CursorStateDev<WW>*)impl_->d_state, (const uint64_t*)impl_->d_words, is_kmer, (uint64_t*)impl_->d_vtab, impl_->vcap);
    });
    rt::stream_sync(s);
    impl_->sought = true;
    bool hn, hp;
    uint32_t st;
    peek(&hn, &hp, &st, nullptr, nullptr);
    check_status(st);
}

void CursorHost::peek(bool* has_next, bool* has_prev, uint32_t* status, uint64_t* out_words, int64_t* out_rec) {
    const int W = eng_.graph->hdr.W;
    rt::stream_t s = eng_.estream();
    with_words(W, [&](auto w_) {
        constexpr int WW = decltype(w_)::value;
        CursorStateDev<WW> h;
        read_state<WW>(impl_->d_state, h, s);
        *has_next = h.has_next != 0; *has_prev = h.has_prev != 0; *status = h.status;
        if (out_words) for (int i = 0; i < WW; i++) out_words[i] = h.out_words[i];
        if (out_rec) *out_rec = h.out_rec;
    });
}

int64_t CursorHost::cur_record() {
    rt::stream_t s = eng_.estream();
    return with_words(eng_.graph->hdr.W, [&](auto w_) {
        CursorStateDev<decltype(w_)::value> h;
        read_state(impl_->d_state, h, s);
        return (int64_t)h.cur.idx;
    });
}

bool CursorHost::has(bool fwd) {
    eng_.enter();
    if (!impl_->sought) return false;
    bool hn, hp; uint32_t st;
    peek(&hn, &hp, &st, nullptr, nullptr);
    return fwd ? hn : hp;
}

// TraversalEngine.assemble(seed) (:112-123): [previous() ... in contig order] + the seed's vertex + [next() ...]
void CursorHost::assemble(const char* seed, int64_t capacity, int64_t* len, uint64_t* words, int64_t* rec) {
    eng_.enter();
    const int W = eng_.graph->hdr.W;
    rt::stream_t s = eng_.estream();
    const int64_t max_len = std::max<int64_t>(0, eng_.cfg.max_branch_length);
    // the cursor's `seen` table holds every vertex stepped onto since the seek (load <= 1/2)
    uint32_t need = 1u << 17;
    while ((uint64_t)need < 2ull * (uint64_t)(max_len + 16)) need <<= 1;
    if (need > impl_->vcap) {
        rt::dfree(impl_->d_vtab);
        impl_->d_vtab = nullptr;
        impl_->d_vtab = rt::dmalloc((size_t)need * 8);
        impl_->vcap = need;
        rt::dmemset(impl_->d_vtab, 0, (size_t)need * 8, s);
    }
    struct Tmp { std::vector<void*> p; ~Tmp() { for (void* x : p) rt::dfree(x); } void* get(size_t nbytes) { void* x = rt::dmalloc(nbytes); p.push_back(x); return x; } } tmp;
    uint64_t* d_w = (uint64_t*)tmp.get((size_t)std::max<int64_t>(1, max_len) * W * 8);
    int64_t* d_r = (int64_t*)tmp.get((size_t)std::max<int64_t>(1, max_len) * 8);
    int64_t* d_n = (int64_t*)tmp.get(16);
    std::vector<uint64_t> part_w[2];
    std::vector<int64_t> part_r[2];
    std::vector<uint64_t> seed_w(W);
    int64_t seed_rec = -1;
    for (int dir = 1; dir >= 0; dir--) {                 // forward first, as the reference does
        seek(seed);
        if (dir == 1) {
            // the seed's own vertex: bases(seed), record(findRecord(seed))
            const bool ok = ascii_to_words(seed, eng_.graph->hdr.k, seed_w.data(), W);
            if (!ok) std::fill(seed_w.begin(), seed_w.end(), 0ull);
            seed_rec = cur_record();                     // (the seek has just looked the seed up)
        }
        with_words(W, [&](auto w_) {
            constexpr int WW = decltype(w_)::value;
            LDBG_LAUNCH(k_cursor_assemble<WW>, 1, 64, s, eng_.view, (CursorStateDev<WW>*)impl_->d_state, dir, (uint64_t*)impl_->d_vtab, impl_->vcap,
                        (LsElem*)impl_->d_ls, impl_->ecap, max_len, d_w, d_r, d_n);
        });
        int64_t hn[2] = {0, 0};
        rt::d2h(hn, d_n, 16, s);
        rt::stream_sync(s);
        check_status((uint32_t)hn[1]);
        part_w[dir].resize((size_t)hn[0] * W);
        part_r[dir].resize((size_t)hn[0]);
        rt::d2h(part_w[dir].data(), d_w, (size_t)hn[0] * W * 8, s);
        rt::d2h(part_r[dir].data(), d_r, (size_t)hn[0] * 8, s);
        rt::stream_sync(s);
    }
    const int64_t nr = (int64_t)part_r[0].size(), nf = (int64_t)part_r[1].size();
    *len = nr + 1 + nf;
    if (capacity < *len) throw StatusError(LDBG_ERR_CAPACITY, "vertex buffers too small: need " + std::to_string(*len));
    for (int64_t i = 0; i < nr; i++) {                   // contig.add(0, cv): the last one stepped onto comes first
        const int64_t from = nr - 1 - i;
        if (words) for (int w = 0; w < W; w++) words[i * W + w] = part_w[0][(size_t)from * W + w];
        if (rec) rec[i] = part_r[0][(size_t)from];
    }
    if (words) for (int w = 0; w < W; w++) words[nr * W + w] = seed_w[(size_t)w];
    if (rec) rec[nr] = seed_rec;
    for (int64_t i = 0; i < nf; i++) {
        if (words) for (int w = 0; w < W; w++) words[(nr + 1 + i) * W + w] = part_w[1][(size_t)i * W + w];
        if (rec) rec[nr + 1 + i] = part_r[1][(size_t)i];
    }
}

void CursorHost::step(bool fwd, char* kmer_out, int64_t* rec_out) {
    eng_.enter();
    const int W = eng_.graph->hdr.W, k = eng_.graph->hdr.k;
    if (!has(fwd))
        throw StatusError(LDBG_ERR_NOSUCHELEMENT, std::string("No single ") + (fwd ? "advance" : "prev") + " kmer from cursor");
    rt::stream_t s = eng_.estream();
    with_words(W, [&](auto w_) {
        constexpr int WW = decltype(w_)::value;
        LDBG_LAUNCH(k_cursor_step<WW>, 1, 64, s, eng_.view, (CursorStateDev<WW>*)impl_->d_state, fwd ? 1 : 0, (uint64_t*)impl_->d_vtab, impl_->vcap, (LsElem*)impl_->d_ls, impl_->ecap);
    });
    rt::stream_sync(s);
    bool hn, hp; uint32_t st;
    std::vector<uint64_t> w(W);
    int64_t rec = -1;
    peek(&hn, &hp, &st, w.data(), &rec);
    check_status(st);
    if (kmer_out) { words_to_ascii(w.data(), k, W, kmer_out); kmer_out[k] = 0; }
    if (rec_out) *rec_out = rec;
}

// ================================================================== cursors in batches (ldbg_engine_cursor_batch)
// A pool of cursor slots in HBM, one per lane: state, `seen` table, link store.  The (seed, direction) items of a batch are a queue; a
// lane takes the next item when its own ends, so no workgroup waits for another.  A batch runs the queue twice: the first pass counts
// (vertices per item, end reason, status), the counts are scanned into CSR offsets, the second pass steps the same cursors again and
// writes every vertex where it belongs (reverse parts reversed).  A cursor is a function of the graph and its seed alone, so both
// passes see the same vertices whichever slot runs an item, and nothing but the result grows with n.
struct CbArgs {
    EngineView e;
    const unsigned char* seeds;      // [n][k] ASCII
    const unsigned char* targets;    // [n][k] ASCII or nullptr
    int64_t n, items, max_steps;
    int direction, colour, deg1;
    // the pool
    void* states;                    // [slots] CursorStateDev<W>
    uint64_t* vtabs;                 // [slots][vcap]
    LsElem* els;                     // [slots][ecap]
    uint32_t* epochs;                // [slots] generation of `seen` the slot's last item ran under
    uint32_t vcap, ecap;
    int64_t slots;
    unsigned long long* ctr;         // [0], [1] queue heads of the two passes, [2] steps of the batch, [3] steps of its longest cursor
    // per seed
    int32_t* nrev; int32_t* nfwd; int64_t* seed_rec;
    uint8_t* end;                    // [2][n] reverse, forward
    uint8_t* item_status;            // [2][n] likewise
    // second pass
    const int64_t* offsets; uint64_t* words; int64_t* rec;
    int pass;
};

// a seed or target as packed words; false: not a k-mer over ACGT (upper case only: the string is looked up, not encoded, kmer.h)
template <int W>
LDBG_DEV bool cb_parse(const unsigned char* c, int k, Kmer<W>& out) {
    const int nw = (k + 31) / 32, lead = W - nw;
    bool bad = false;
    int i = 0;
#pragma unroll
    for (int wi = 0; wi < W; wi++) {
        uint64_t acc = 0;
        if (wi >= lead) {
            const int cnt = wi == lead ? k - 32 * (nw - 1) : 32;
            for (int j = 0; j < cnt; j++) {
                const unsigned ch = c[i++];
                const unsigned v = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : 3u;
                bad |= !(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
                acc = (acc << 2) | (uint64_t)v;
            }
        }
        out.w[wi] = acc;
    }
    if (bad) for (int wi = 0; wi < W; wi++) out.w[wi] = 0ull;
    return !bad;
}

// the loop bodies of ComputeInheritance.callVariant (:129,141,160) and ComputeAssemblyQuality.callVariant (:114,126,145) on the vertex just
// stepped onto -> 0 go on, 1 stop, 2 the reference's NullPointerException (no record under a colour rule)
template <int W>
LDBG_DEV int cb_stop_test(const CbArgs& a, bool fwd, const Kmer<W>& tk, int64_t rec, bool has_target, const Kmer<W>& target) {
    if (a.colour >= 0) {
        if (rec < 0) return 2;
        if ((int32_t)graph_cov(a.e.g, rec, a.colour) > 0) {                 // getCoverage(c) > 0 on the Java int (Q5)
            if (!a.deg1) return 1;
            const uint32_t ed = graph_edges(a.e.g, rec, a.colour);
            const bool same = kmer_eq<W>(tk, graph_key<W>(a.e.g, rec));      // getKmerAsString().equals(getCanonicalKmer().getKmerAsString())
            const int in_deg = popc4(ed >> 4), out_deg = popc4(ed & 0xFu);
            if ((fwd == same ? in_deg : out_deg) == 1) return 1;
        }
    }
    return has_target && kmer_eq<W>(tk, target) ? 1 : 0;
}

template <int W>
LDBG_DEV void cursor_batch_item(const CbArgs& a, int64_t slot, int64_t item) {
    const EngineView& e = a.e;
    const bool both = a.direction == LDBG_DIR_BOTH;
    const int64_t i = both ? item >> 1 : item;
    const bool fwd = both ? (item & 1) != 0 : a.direction == LDBG_DIR_FORWARD;
    CursorStateDev<W>& st = ((CursorStateDev<W>*)a.states)[slot];
    uint64_t* vtab = a.vtabs + (size_t)slot * a.vcap;
    LsElem* els = a.els + (size_t)slot * a.ecap;
    // a new item on the slot is a new epoch of its `seen` table; the table is swept when the epochs wrap around, and when the slots claimed
    // since the last sweep leave this item less room than it can claim (three at the seek and one per step) below a load of 3/4 — a sweep
    // comes after vcap / 4 claims at the least, so sweeping costs a claim four writes at the most
    uint32_t epoch = a.epochs[slot] + 1u;
    if (epoch > LDBG_VT_EPOCH_MAX || (uint64_t)st.vt_used + (uint64_t)a.max_steps + 16ull > (uint64_t)(a.vcap / 4u) * 3ull) {
        for (uint32_t q = 0; q < a.vcap; q++) LDBG_GLOBAL(uint64_t, vtab)[q] = 0ull;
        st.vt_used = 0;
        epoch = 1;
    }
    a.epochs[slot] = epoch;
    Kmer<W> sk, target;
    for (int w = 0; w < W; w++) target.w[w] = 0ull;
    const bool is_kmer = cb_parse<W>(a.seeds + (size_t)i * (size_t)e.g.k, e.g.k, sk);
    const bool has_target = a.targets ? cb_parse<W>(a.targets + (size_t)i * (size_t)e.g.k, e.g.k, target) : false;
    if (is_kmer) node_find<W>(e, sk, st.cur);
    else node_null(e, st.cur);
    for (int w = 0; w < W; w++) st.cur_words[w] = sk.w[w];
    st.go_forward = fwd ? 1 : 0;
    cs_reseek<W, true>(e, st, vtab, a.vcap);              // seek(seed)
    const int64_t seed_rec = st.cur.idx;
    int64_t base = 0;
    if (a.pass == 1) {
        base = a.offsets[i] + (fwd ? (int64_t)a.nrev[i] + (both ? 1 : 0) : (int64_t)a.nrev[i] - 1);
        if (both && fwd) {                                // the seed's own vertex: bases(seed), record(findRecord(seed))
            const int64_t at = a.offsets[i] + a.nrev[i];
            for (int w = 0; w < W; w++) a.words[at * W + w] = sk.w[w];
            a.rec[at] = seed_rec;
        }
    }
    int64_t cnt = 0;
    uint32_t status = st.status;
    uint32_t reason = LDBG_CURSOR_FAILED;
    if (status == ST_OK) {
        bool has = (fwd ? st.has_next : st.has_prev) != 0;
        reason = has ? LDBG_CURSOR_LIMIT : LDBG_CURSOR_END;
        while (has && cnt < a.max_steps) {
            cs_step<W, true>(e, st, fwd, vtab, a.vcap, els, a.ecap, epoch);
            status = st.status;
            if (status != ST_OK) { reason = LDBG_CURSOR_FAILED; break; }
            Kmer<W> tk;
            for (int w = 0; w < W; w++) tk.w[w] = st.out_words[w];
            const int64_t rec = st.out_rec;
            if (a.pass == 1) {                            // contig.add(cv) / contig.add(0, cv)
                const int64_t at = fwd ? base + cnt : base - cnt;
                for (int w = 0; w < W; w++) a.words[at * W + w] = tk.w[w];
                a.rec[at] = rec;
            }
            cnt++;
            const int sr = cb_stop_test<W>(a, fwd, tk, rec, has_target, target);
            if (sr == 2) { status = ST_NULLPTR; reason = LDBG_CURSOR_FAILED; break; }
            if (sr == 1) { reason = LDBG_CURSOR_STOP; break; }
            has = (fwd ? st.has_next : st.has_prev) != 0;
            reason = has ? LDBG_CURSOR_LIMIT : LDBG_CURSOR_END;
        }
    }
    if (a.pass == 0) {
        (fwd ? a.nfwd : a.nrev)[i] = (int32_t)cnt;
        a.end[(fwd ? a.n : 0) + i] = (uint8_t)reason;
        a.item_status[(fwd ? a.n : 0) + i] = (uint8_t)(status == ST_OK ? LDBG_CURSOR_OK : status == ST_NULLPTR ? LDBG_CURSOR_NULLPOINTER : LDBG_CURSOR_CAPACITY);
        if (fwd || !both) a.seed_rec[i] = seed_rec;
        atomic_add_u64(a.ctr + 2, (unsigned long long)cnt);
        atomic_max_u32((unsigned*)(a.ctr + 3), (unsigned)cnt);
    }
}

// one cursor slot per lane; the lanes of the pool drain the queue of items
template <int W>
LDBG_WAVE_KERNEL void k_cursor_batch(CbArgs a) {
    const int64_t slot = global_tid();
    if (slot >= a.slots) return;
    while (true) {
        const int64_t item = (int64_t)atomic_add_u64(a.ctr + a.pass, 1ull);
        if (item >= a.items) break;
        cursor_batch_item<W>(a, slot, item);
    }
}

// per seed after the first pass: its vertices (for the scan) and its status (the reverse direction's first, as the loops run in that
// order in callVariant); *total = all vertices as 64 bits (the scan counts modulo 2^32)
LDBG_KERNEL void k_cursor_counts(int64_t n, int both, const int32_t* nrev, const int32_t* nfwd, const uint8_t* item_status, uint8_t* status, uint32_t* cnt,
                                 unsigned long long* total) {
    unsigned long long sum = 0;
    for (int64_t i = global_tid(); i < n; i += global_nthreads()) {
        const uint32_t c = (uint32_t)nrev[i] + (uint32_t)nfwd[i] + (both ? 1u : 0u);
        cnt[i] = c;
        sum += c;
        status[i] = item_status[i] != LDBG_CURSOR_OK ? item_status[i] : item_status[n + i];
    }
    if (sum) atomic_add_u64(total, sum);
}
LDBG_KERNEL void k_cursor_offsets(int64_t n, const uint32_t* off32, int64_t* offsets) {
    for (int64_t i = global_tid(); i <= n; i += global_nthreads()) offsets[i] = (int64_t)off32[i];
}

CursorBatchResult::~CursorBatchResult() {
    for (void* p : {d_offsets, d_words, d_rec, d_nrev, d_nfwd, d_seed_rec, d_end, d_status}) rt::dfree(p);
}
void CursorBatchResult::get(void* offsets, void* words, void* rec, void* nrev, void* nfwd, void* seed_rec, void* end_rev, void* end_fwd, void* status,
                            bool on_device, rt::stream_t s) const {
    rt::set_device(device);
    auto copy = [&](void* dst, const void* src, size_t bytes) {
        if (!dst || !bytes) return;
        if (on_device) rt::d2d(dst, src, bytes, s); else rt::d2h(dst, src, bytes, s);
    };
    copy(offsets, d_offsets, (size_t)(n + 1) * 8);
    copy(words, d_words, (size_t)total * (size_t)W * 8);
    copy(rec, d_rec, (size_t)total * 8);
    copy(nrev, d_nrev, (size_t)n * 4);
    copy(nfwd, d_nfwd, (size_t)n * 4);
    copy(seed_rec, d_seed_rec, (size_t)n * 8);
    copy(end_rev, d_end, (size_t)n);
    copy(end_fwd, (const uint8_t*)d_end + n, (size_t)n);
    copy(status, d_status, (size_t)n);
    if (!on_device) rt::stream_sync(s);
}

struct CursorBatchHost::Impl {
    void* d_states = nullptr; void* d_vtabs = nullptr; void* d_els = nullptr; void* d_epochs = nullptr; void* d_ctr = nullptr;
    uint32_t vcap = 0, ecap = 256;
    int64_t slots = 0, asked = 0;     // asked: the slots the pool was built for, before the memory budget cut them
    size_t state_bytes = 0;
    void release() {
        rt::dfree(d_states); rt::dfree(d_vtabs); rt::dfree(d_els); rt::dfree(d_epochs);
        d_states = d_vtabs = d_els = d_epochs = nullptr;
        slots = asked = 0;
    }
};

CursorBatchHost::CursorBatchHost(Engine& e) : eng_(e), impl_(new Impl) {
    impl_->state_bytes = with_words(e.graph->hdr.W, [](auto w_) { return sizeof(CursorStateDev<decltype(w_)::value>); });
}
CursorBatchHost::~CursorBatchHost() {
    eng_.quiesce();
    impl_->release();
    rt::dfree(impl_->d_ctr);
    delete impl_;
}

// The pool: as many slots as the batch has items, at most one per lane the device holds at eight wavefronts per SIMD lane slot, at most
// what 40 % of the free memory pays for (the engine's convention, walk.cpp), at most LDBG_CURSOR_SLOTS (a test hook read here, as
// LDBG_IMG_YIELD is).  A pool that is large enough is kept; its tables carry on under their epochs.
void CursorBatchHost::ensure_pool(uint32_t vcap, int64_t items) {
    Impl& p = *impl_;
    const size_t slot_bytes = p.state_bytes + (size_t)vcap * 8 + (size_t)p.ecap * sizeof(LsElem) + 4;
    int64_t cap = (int64_t)rt::cu_count(eng_.graph->device) * 8 * 64;
#ifdef LDBG_HOSTSIM
    cap = 4096;                                  // (threads of a simulated launch)
#endif
    if (const char* ev = getenv("LDBG_CURSOR_SLOTS")) cap = std::max<int64_t>(1, std::min<int64_t>(cap, atoll(ev)));
    int64_t want = std::min<int64_t>(cap, std::max<int64_t>(64, (int64_t)next_pow2((uint64_t)std::min<int64_t>(items, (int64_t)1 << 30))));
    if (p.slots > 0 && p.vcap == vcap && p.asked >= want) return;
    eng_.quiesce();
    p.release();
    size_t free_b = 0, total_b = 0;
    rt::mem_info(&free_b, &total_b);
    const int64_t afford = (int64_t)((double)free_b * 0.40 / (double)slot_bytes);
    if (afford < 1) throw StatusError(LDBG_ERR_HIP, "cursor batch: no device memory for one cursor slot of " + std::to_string(slot_bytes) + " bytes");
    p.asked = want;
    want = std::min<int64_t>(want, afford);
    rt::stream_t s = eng_.estream();
    p.d_states = rt::dmalloc((size_t)want * p.state_bytes);
    p.d_vtabs = rt::dmalloc((size_t)want * vcap * 8);
    p.d_els = rt::dmalloc((size_t)want * p.ecap * sizeof(LsElem));
    p.d_epochs = rt::dmalloc((size_t)want * 4);
    rt::dmemset(p.d_states, 0, (size_t)want * p.state_bytes, s);
    rt::dmemset(p.d_vtabs, 0, (size_t)want * vcap * 8, s);
    // test hook: the epoch the slots start from (the 14-bit epochs wrap around after 16,383 items on a slot)
    uint32_t epoch0 = 0;
    if (const char* ev = getenv("LDBG_CURSOR_EPOCH0")) epoch0 = (uint32_t)std::max<long long>(0, std::min<long long>(atoll(ev), LDBG_VT_EPOCH_MAX));
    std::vector<uint32_t> ep((size_t)want, epoch0);
    rt::h2d(p.d_epochs, ep.data(), (size_t)want * 4, s);
    rt::stream_sync(s);
    p.vcap = vcap; p.slots = want;
}

CursorBatchResult* CursorBatchHost::run(const char* seeds, int64_t n, bool on_device, int direction, int64_t max_steps, const ldbg_cursor_stop* stop) {
    Engine& eng = eng_;
    check_whole_table(*eng.graph, "cursor batch");
    const int W = eng.graph->hdr.W, k = eng.graph->hdr.k, C = eng.graph->hdr.C;
    if (n < 0) throw StatusError(LDBG_ERR_ARG, "cursor batch: n < 0");
    if (direction != LDBG_DIR_BOTH && direction != LDBG_DIR_FORWARD && direction != LDBG_DIR_REVERSE) throw StatusError(LDBG_ERR_ARG, "cursor batch: unknown direction");
    if (n > 0 && !seeds) throw StatusError(LDBG_ERR_ARG, "cursor batch: null seeds");
    if (stop && stop->colour >= C) throw StatusError(LDBG_ERR_ARG, "cursor batch: colour " + std::to_string(stop->colour) + " of a graph of " + std::to_string(C));
    if (max_steps <= 0) max_steps = std::max<int64_t>(0, eng.cfg.max_branch_length);
    if (max_steps > ((int64_t)1 << 20)) throw StatusError(LDBG_ERR_ARG, "cursor batch: max_steps above 2^20 (1048576)");
    if (n > (((int64_t)1 << 31) - 1) / 2) throw StatusError(LDBG_ERR_UNSUPPORTED, "cursor batch: 2^30 seeds or more in one call");
    eng.enter();
    rt::stream_t s = eng.estream();
    std::unique_ptr<CursorBatchResult> res(new CursorBatchResult);
    res->device = eng.graph->device; res->W = W; res->n = n;
    res->d_offsets = rt::dmalloc((size_t)(n + 1) * 8);
    if (n == 0) {
        rt::dmemset(res->d_offsets, 0, 8, s);
        rt::stream_sync(s);
        return res.release();
    }
    const bool both = direction == LDBG_DIR_BOTH;
    const int64_t items = both ? 2 * n : n;
    // the `seen` table of a slot: today's load rule (CursorHost::assemble), without its floor
    const uint32_t vcap = next_pow2(2ull * (uint64_t)(max_steps + 16));
    ensure_pool(vcap, items);
    Impl& p = *impl_;
    if (!p.d_ctr) p.d_ctr = rt::dmalloc(5 * 8);
    struct Tmp { std::vector<void*> v; ~Tmp() { for (void* x : v) rt::tfree(x); } void* get(size_t b) { void* x = rt::tmalloc(b); v.push_back(x); return x; } } tmp;
    const unsigned char* d_seeds = (const unsigned char*)seeds;
    const unsigned char* d_targets = stop ? (const unsigned char*)stop->targets : nullptr;
    if (!on_device) {
        void* ds = tmp.get((size_t)n * k);
        rt::h2d(ds, seeds, (size_t)n * k, s);
        d_seeds = (const unsigned char*)ds;
        if (d_targets) {
            void* dt = tmp.get((size_t)n * k);
            rt::h2d(dt, stop->targets, (size_t)n * k, s);
            d_targets = (const unsigned char*)dt;
        }
    }
    res->d_nrev = rt::dmalloc((size_t)n * 4); res->d_nfwd = rt::dmalloc((size_t)n * 4);
    res->d_seed_rec = rt::dmalloc((size_t)n * 8);
    res->d_end = rt::dmalloc((size_t)n * 2); res->d_status = rt::dmalloc((size_t)n);
    uint8_t* d_item_status = (uint8_t*)tmp.get((size_t)n * 2);
    const int64_t nchunks = (n + LDBG_SCAN_CHUNK - 1) / LDBG_SCAN_CHUNK;
    uint32_t* d_cnt = (uint32_t*)tmp.get((size_t)n * 4);
    uint32_t* d_off32 = (uint32_t*)tmp.get((size_t)(n + 1) * 4);
    uint32_t* d_sums = (uint32_t*)tmp.get((size_t)(nchunks + 1) * 4);
    uint32_t* d_offs = (uint32_t*)tmp.get((size_t)(nchunks + 1) * 4);
    rt::dmemset(res->d_nrev, 0, (size_t)n * 4, s); rt::dmemset(res->d_nfwd, 0, (size_t)n * 4, s);
    rt::dmemset(res->d_end, 0, (size_t)n * 2, s); rt::dmemset(d_item_status, 0, (size_t)n * 2, s);     // (LDBG_CURSOR_END, LDBG_CURSOR_OK: a direction not asked for)
    rt::dmemset(p.d_ctr, 0, 5 * 8, s);
    CbArgs a{};
    a.e = eng.view;
    a.seeds = d_seeds; a.targets = d_targets;
    a.n = n; a.items = items; a.max_steps = max_steps;
    a.direction = direction; a.colour = stop ? std::max(-1, stop->colour) : -1; a.deg1 = stop && stop->arrival_degree_one ? 1 : 0;
    a.states = p.d_states; a.vtabs = (uint64_t*)p.d_vtabs; a.els = (LsElem*)p.d_els; a.epochs = (uint32_t*)p.d_epochs;
    a.vcap = p.vcap; a.ecap = p.ecap; a.slots = std::min<int64_t>(p.slots, items);
    a.ctr = (unsigned long long*)p.d_ctr;
    a.nrev = (int32_t*)res->d_nrev; a.nfwd = (int32_t*)res->d_nfwd; a.seed_rec = (int64_t*)res->d_seed_rec;
    a.end = (uint8_t*)res->d_end; a.item_status = d_item_status;
    a.pass = 0;
    const int grid = (int)((a.slots + 63) / 64);
    rt::Event e0, e1, e2, e3;
    e0.record(s);
    LDBG_LAUNCH_W(W, k_cursor_batch, grid, 64, s, a);
    LDBG_LAUNCH(k_cursor_counts, grid_for(n), 256, s, n, both ? 1 : 0, (const int32_t*)res->d_nrev, (const int32_t*)res->d_nfwd, (const uint8_t*)d_item_status,
                (uint8_t*)res->d_status, d_cnt, (unsigned long long*)p.d_ctr + 4);
    scan_u32(d_cnt, n, d_off32, d_sums, d_offs, s);
    LDBG_LAUNCH(k_cursor_offsets, grid_for(n + 1), 256, s, n, (const uint32_t*)d_off32, (int64_t*)res->d_offsets);
    e1.record(s);
    unsigned long long ctr[5];
    rt::d2h(ctr, p.d_ctr, sizeof(ctr), s);
    rt::stream_sync(s);
    if (ctr[4] >= (1ull << 32)) throw StatusError(LDBG_ERR_UNSUPPORTED, "cursor batch: 2^32 vertices or more in one result (" + std::to_string(ctr[4]) + "); split the batch");
    res->total = (int64_t)ctr[4];
    res->d_words = rt::dmalloc((size_t)std::max<int64_t>(1, res->total) * W * 8);
    res->d_rec = rt::dmalloc((size_t)std::max<int64_t>(1, res->total) * 8);
    a.offsets = (const int64_t*)res->d_offsets; a.words = (uint64_t*)res->d_words; a.rec = (int64_t*)res->d_rec;
    a.pass = 1;
    e2.record(s);
    LDBG_LAUNCH_W(W, k_cursor_batch, grid, 64, s, a);
    e3.record(s);
    rt::stream_sync(s);
    profile_add("cursor", rt::Event::elapsed_ms(e0, e1) + rt::Event::elapsed_ms(e2, e3));
    profile_add("cursor_steps", (double)ctr[2]);
    profile_add("cursor_longest", (double)(ctr[3] & 0xFFFFFFFFull));
    return res.release();
}

}  // namespace ldbg
