// Graph construction on the device: sequences of several samples -> the sorted multi-colour table, as
// TempGraphAssembler.buildGraph (J/utils/assembler/TempGraphAssembler.java:19-127) builds it record by record in a TreeMap.
#pragma once
#include <string>
#include <vector>

#include "devmem.h"
#include "graph.h"

namespace ldbg {

#define LDBG_BUILD_CHUNK 4096       // sorted windows per chunk: the stretch one wavefront marks and reduces, one entry of the scanned counts

// the built table: the header CortexGraphWriter writes for it and the records in the file's layout (8W + 5C bytes each, k-mer order)
// back to back in device memory (nullptr when there is no record)
struct BuiltRecords {
    CtxHeader hdr;
    std::vector<uint8_t> header;
    DevRecords d_records;
    int64_t N = 0;
    int device = 0;
};

BuiltRecords build_records(const ldbg_build_sample* samples, int n_samples, int k, int flags, int device);
// header, then the records downloaded once
void build_write_ctx(const BuiltRecords& b, const std::string& out_path);

}  // namespace ldbg
