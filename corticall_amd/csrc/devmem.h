// Host-side owners of what a batch lane borrows from the device (both builds): its temporaries, its packed records, a stream and a timer of
// its own, and the one writer of "header, then packed records" files.  Everything here lets go on every way out of a scope, a throw included.
#pragma once
#include <stdio.h>

#include <memory>

#include "rt.h"

namespace ldbg {

struct DevBlocks {             // device blocks of one call, or of one object as a member: freed on every way out
    std::vector<void*> p;
    DevBlocks() = default;
    DevBlocks(const DevBlocks&) = delete;
    DevBlocks& operator=(const DevBlocks&) = delete;
    ~DevBlocks() { clear(); }
    template <class T>
    T* get(size_t n) { p.push_back(nullptr); p.back() = rt::dmalloc(n * sizeof(T)); return (T*)p.back(); }
    void drop(void* x) { for (void*& y : p) if (y == x) { rt::dfree(y); y = nullptr; } }
    void clear() { for (void* x : p) rt::dfree(x); p.clear(); }
};

// packed records (or any bytes) in device memory that travel between functions: freed by the last holder
struct DevFree { void operator()(void* p) const { rt::dfree(p); } };
typedef std::unique_ptr<uint8_t, DevFree> DevRecords;

struct OwnStream {             // a stream of the current device for one call
    rt::stream_t s = rt::stream_create();
    OwnStream() = default;
    OwnStream(const OwnStream&) = delete;
    OwnStream& operator=(const OwnStream&) = delete;
    ~OwnStream() { rt::stream_destroy(s); }
};

struct DevTimer {              // device time of the stretches of launches between two waits of the host
    rt::Event a, b;
    double ms = 0;
    void begin(rt::stream_t s) { a.record(s); }
    void end(rt::stream_t s) { b.record(s); ms += rt::Event::elapsed_ms(a, b); }
};

// hdr, then the `total` bytes at d_records (memory of `device`), downloaded through a pinned buffer of at most 64 MB
inline void write_records_file(const std::vector<uint8_t>& hdr, const uint8_t* d_records, size_t total, int device, rt::stream_t stream, const std::string& path) {
    struct File {
        FILE* f;
        ~File() { if (f) fclose(f); }
    } out{fopen(path.c_str(), "wb")};
    if (!out.f) throw StatusError(LDBG_ERR_CORTEXJDK, "Unable to open file '" + path + "'");
    const size_t step = (size_t)64 << 20;
    std::unique_ptr<void, void (*)(void*)> pin(nullptr, rt::hfree_pinned);
    bool ok = fwrite(hdr.data(), 1, hdr.size(), out.f) == hdr.size();
    if (total) {
        rt::set_device(device);
        pin.reset(rt::hmalloc_pinned(std::min(total, step)));
    }
    for (size_t o = 0; o < total && ok; o += step) {
        const size_t nb = std::min(step, total - o);
        rt::d2h(pin.get(), d_records + o, nb, stream);
        rt::stream_sync(stream);
        ok = fwrite(pin.get(), 1, nb, out.f) == nb;
    }
    ok = fclose(out.f) == 0 && ok;
    out.f = nullptr;
    if (!ok) throw StatusError(LDBG_ERR_CORTEXJDK, "Unable to write record to file '" + path + "'");
}

}  // namespace ldbg
