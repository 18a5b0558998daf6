// Link construction on the device: the reads of one sample threaded through a resident graph -> the link records
// TempLinksAssembler.buildLinks (J/utils/assembler/TempLinksAssembler.java:29-182) collects in a HashMap of HashSets, in the order
// and the text in which it writes them.
#pragma once
#include <string>
#include <vector>

#include "links.h"

namespace ldbg {

// -> BuiltLinks (links.h).  reads: one text buffer and n_reads + 1 offsets, as ldbg_build_sample passes sequences
BuiltLinks build_links(const Graph& g, const char* sample_name, const char* bases, const int64_t* offsets, int64_t n_reads, int flags);
// the decompressed text of the file: constructLinksHeader(...).toString(8), two newlines, the records, a newline
std::string built_links_text(const BuiltLinks& b);
void built_links_write(const BuiltLinks& b, const std::string& out_path);

}  // namespace ldbg
