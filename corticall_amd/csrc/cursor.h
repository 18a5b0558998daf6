#pragma once
#include "engine_host.h"

namespace ldbg {

// host handle of the device-resident cursor of one engine (TraversalEngine.java:241-339)
class CursorHost {
public:
    explicit CursorHost(Engine& e);
    ~CursorHost();
    void seek(const char* kmer);
    bool has(bool fwd);
    void step(bool fwd, char* kmer_out, int64_t* rec_out);
    // assemble(seed) (TraversalEngine.java:112-145): vertices in contig order (packed k-mer words, record index or -1)
    void assemble(const char* seed, int64_t capacity, int64_t* len, uint64_t* words, int64_t* rec);

private:
    struct Impl;
    Engine& eng_;
    Impl* impl_;
    void peek(bool* has_next, bool* has_prev, uint32_t* status, uint64_t* out_words, int64_t* out_rec);
    static void check_status(uint32_t st);
    int64_t cur_record();
};

// result of one cursor batch (ldbg_engine_cursor_batch), resident in HBM until it is asked for
struct CursorBatchResult {
    int device = 0, W = 0;
    int64_t n = 0, total = 0;
    void* d_offsets = nullptr;     // [n + 1] int64
    void* d_words = nullptr;       // [total][W] u64
    void* d_rec = nullptr;         // [total] int64
    void* d_nrev = nullptr;        // [n] int32
    void* d_nfwd = nullptr;        // [n] int32
    void* d_seed_rec = nullptr;    // [n] int64
    void* d_end = nullptr;         // [2][n] u8: reverse, forward
    void* d_status = nullptr;      // [n] u8
    ~CursorBatchResult();
    // any pointer may be null; on_device: the destinations are in this device's memory and the copies are queued on s
    void get(void* offsets, void* words, void* rec, void* nrev, void* nfwd, void* seed_rec, void* end_rev, void* end_fwd, void* status, bool on_device,
             rt::stream_t s) const;
};

// n cursors advanced to their end by a pool of cursor slots; the pool is kept from batch to batch
class CursorBatchHost {
public:
    explicit CursorBatchHost(Engine& e);
    ~CursorBatchHost();
    CursorBatchResult* run(const char* seeds, int64_t n, bool on_device, int direction, int64_t max_steps, const ldbg_cursor_stop* stop);

private:
    struct Impl;
    Engine& eng_;
    Impl* impl_;
    void ensure_pool(uint32_t vcap, int64_t items);
};

}  // namespace ldbg
