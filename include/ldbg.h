/* ldbg.h — C ABI of libldbg.so, the MI355X-native LdBG traversal engine.
 *
 * This is the drop-in boundary for ONE hot path of mcveanlab/Corticall: CortexGraph record
 * iteration, binary-search random access (findRecord) and the link-guided walk / DFS of
 * TraversalEngine.  The reference has no FFI for this path; the seam is two Java interfaces
 * and one façade, so every entry point below cites the Java member it replaces
 * (J/ = public/java/src/uk/ac/ox/well/cortexjdk/).  A JNI / ctypes binding calls exactly
 * these functions.
 *
 * Conventions
 *   - every function returns an ldbg_status; on failure ldbg_last_error() (thread-local)
 *     holds the message the reference would have put in its exception.
 *   - k-mers cross the boundary either as ASCII (n × k bytes, no terminators) or as
 *     "packed words": W = ceil(k/32) uint64 per k-mer, word 0 most significant, 2 bits per
 *     base (A=0,C=1,G=2,T=3), right aligned — the value McCortex stores in a .ctx record
 *     (docs/ctx_spec.md "Binary kmer specification").
 *   - plain pointers and sizes only; "_dev" variants take device pointers (HBM resident
 *     inputs/outputs) and a hipStream_t passed as void*; all others take host pointers.
 *   - handles are not thread-safe (neither are the reference's objects); distinct handles
 *     may be used from distinct threads.
 *   - there is NO CPU fallback: every call that computes runs HIP kernels on the handle's
 *     device and fails with LDBG_ERR_HIP when no GPU is present.
 */
#ifndef LDBG_H
#define LDBG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    LDBG_OK = 0,
    LDBG_ERR_CORTEXJDK = 1,      /* J/utils/exceptions/CortexJDKException (bad magic/version/unsorted/IO/config) */
    LDBG_ERR_NULLPOINTER = 2,    /* input on which the reference throws NullPointerException */
    LDBG_ERR_NOSUCHELEMENT = 3,  /* TraversalEngine.next()/previous() without a successor (TraversalEngine.java:242,282) */
    LDBG_ERR_UNSUPPORTED = 4,
    LDBG_ERR_HIP = 5,            /* no device / HIP runtime failure */
    LDBG_ERR_ARG = 6,
    LDBG_ERR_CAPACITY = 7        /* caller-provided output buffer too small; required size is reported */
} ldbg_status;

typedef struct ldbg_graph ldbg_graph;     /* DeBruijnGraph backed by a .ctx file, resident in HBM */
typedef struct ldbg_links ldbg_links;     /* ConnectivityAnnotations (.ctp.gz), resident in HBM */
typedef struct ldbg_engine ldbg_engine;   /* TraversalEngine */
typedef struct ldbg_dfs_result ldbg_dfs_result;

const char* ldbg_last_error(void);
const char* ldbg_version(void);
/* number of visible HIP devices (0 on a CPU-only host; no compute entry point works then) */
ldbg_status ldbg_device_count(int* count);

/* ------------------------------------------------------------------ k-mer helpers (host, no GPU needed)
 * CortexRecord.encodeBinaryKmer / decodeBinaryKmer (J/utils/io/graph/cortex/CortexRecord.java:291-334) */
ldbg_status ldbg_kmer_encode(const char* ascii, int k, uint64_t* words_out);
ldbg_status ldbg_kmer_decode(const uint64_t* words, int k, char* ascii_out /* k bytes + NUL */);

/* Sort (J/commands/utils/Sort.java:20-49): writes the records of in_path in k-mer order (CortexRecord.compareTo :210-212,
 * stable like Arrays.sort) under the unchanged header — produces the sorted table ldbg_graph_open requires.  The order is
 * computed by a radix sort on the device. */
ldbg_status ldbg_sort_ctx(const char* in_path, const char* out_path, int device, int64_t* num_records);
/* Join (J/commands/utils/Join.java:16-60; CortexCollection.java:34-58, 218-293): the union of the k-mers of several sorted
 * graphs with every graph's colours side by side, written as one graph.  num_records = k-mers written. */
ldbg_status ldbg_join_ctx(const char* const* in_paths, int n_paths, const char* out_path, int device, int64_t* num_records);
/* CortexGraphWriter over a selection of records (J/utils/io/graph/cortex/CortexGraphWriter.java:40-135, as the filters use it:
 * setHeader(in.getHeader()), addRecord for the chosen records in the order given, close — FindTips.java:112-131).  A file
 * operation on the host. */
ldbg_status ldbg_ctx_write_records(const char* in_path, const int64_t* indices, int64_t n, const char* out_path);

/* ------------------------------------------------------------------ graph: G1-G3
 * new CortexGraph(path)              J/utils/io/graph/cortex/CortexGraph.java:40-48, 66-168
 * The file is parsed on the host, streamed to the device, verified strictly ascending
 * (the reference asserts sortedness lazily at :295-301) and laid out in HBM. */
ldbg_status ldbg_graph_open(const char* path, int device, ldbg_graph** out);
/* same, from an in-memory image of a .ctx file (header + records) */
ldbg_status ldbg_graph_open_memory(const void* image, int64_t nbytes, int device, ldbg_graph** out);
/* same, the header bytes on the host and the records (sorted, the file's record layout) already in DEVICE memory: a shard of a
 * hash-partitioned table cut on the device (corticall_amd/distributed.py) is laid out without a round trip through the host */
ldbg_status ldbg_graph_open_device(const void* header, int64_t header_bytes, const void* d_records, int64_t n_records, int device, ldbg_graph** out);
/* TempGraphAssembler.buildGraph (J/utils/assembler/TempGraphAssembler.java:19-127): the sorted multi-colour graph of the sequences of
 * an ordered list of samples, built on the device.  Colour c is sample c.  Every sequence is upper-cased; every
 * window sk = seq[i, i + k) counts once in cov[c] (a Java int: it wraps) of canon = min(sk, revcomp(sk)) and ORs the neighbouring
 * bases seq[i - 1] and seq[i + k] into the record's edges of colour c, complemented and swapped when revcomp(sk) < sk (a
 * palindrome is not flipped; the orientation is decided by value, not by CanonicalKmer's hash test).  A sequence shorter
 * than k adds nothing; a sample without windows is still a colour.  Header: version 6, zero read length and total sequence, empty
 * cleaning block.  A byte other than ACGTacgt inside a sequence of k bytes or more: LDBG_ERR_CORTEXJDK (the reference throws when it
 * encodes such a k-mer).  LDBG_BUILD_SPLIT_NON_ACGT (an EXTENSION, not the reference's behaviour): every such byte cuts its sequence
 * in two instead - no window holds it, no edge crosses it (FASTA with runs of N).
 * LDBG_ERR_ARG: k outside 3..128, no samples or more than LDBG_MAX_COLORS, two samples of one name, a null pointer, decreasing
 * offsets.  LDBG_ERR_UNSUPPORTED: 2^32 or more windows in one call. */
typedef struct {
    const char* sample_name;
    const char* bases;          /* the sample's sequences back to back: sequence i is bases[offsets[i], offsets[i + 1]) */
    const int64_t* offsets;     /* n_sequences + 1 entries, not decreasing */
    int64_t n_sequences;
} ldbg_build_sample;
#define LDBG_BUILD_SPLIT_NON_ACGT 1
/* the graph resident on the device, as ldbg_graph_open would lay out the file ldbg_graph_build_ctx writes; no file is written */
ldbg_status ldbg_graph_build(const ldbg_build_sample* samples, int n_samples, int k, int flags, int device, ldbg_graph** out);
/* the same graph written to out_path (the records cross the bus once); num_records (may be NULL) = k-mers written */
ldbg_status ldbg_graph_build_ctx(const ldbg_build_sample* samples, int n_samples, int k, int flags, int device, const char* out_path, int64_t* num_records);
/* new CortexCollection(graphs...)   J/utils/io/graph/cortex/CortexCollection.java:34-58: several sorted graphs of one k-mer size as ONE
 * graph, every member's colours side by side, merged on the device without writing a file.  find_view = 0: the records its
 * iterator yields (:218-293, the union of the members' k-mers); find_view = 1: the graph its findRecord answers from (:160-188, one
 * findRecord per member — a member of two records or fewer never finds anything).  Engines are created on the find
 * view; the two differ only when such a member is present. */
ldbg_status ldbg_graph_open_collection(const char* const* paths, int n_paths, int find_view, int device, ldbg_graph** out);
ldbg_status ldbg_graph_close(ldbg_graph* g);                                     /* DeBruijnGraph.close() */
/* getKmerSize/getKmerBits/getNumColors/getNumRecords/getVersion   CortexGraph.java:325-335 */
ldbg_status ldbg_graph_info(const ldbg_graph* g, int* k, int* W, int* C, int64_t* N, int* version);
ldbg_status ldbg_graph_device(const ldbg_graph* g, int* device);
/* A shard of a hash-partitioned table (corticall_amd/distributed.py) must answer membership exactly: quirk Q1
 * (findRecord never finds anything in a graph of <= 2 records, CortexGraph.java:274-282) is a property of the whole
 * graph and is applied by the partitioned front end.  is_shard != 0 turns Q1 off for this handle. */
ldbg_status ldbg_graph_set_shard(ldbg_graph* g, int is_shard);
/* getSampleName(color) / getColor(color)                          CortexGraph.java:329,335 */
ldbg_status ldbg_graph_sample_name(const ldbg_graph* g, int color, char* buf, int buflen);
typedef struct {
    uint32_t mean_read_length;
    uint64_t total_sequence;            /* as the reference reads it (big-endian) */
    uint8_t tip_clipping, low_covg_supernodes_removed, low_covg_kmers_removed, cleaned_against_graph;
    uint32_t low_cov_supernodes_threshold, low_cov_kmer_threshold;
} ldbg_color_info;
ldbg_status ldbg_graph_color_info(const ldbg_graph* g, int color, ldbg_color_info* out,
                                  char* cleaned_against_name, int buflen);
/* getColorForSampleName(name)                                     CortexGraph.java:337-357 ; -1 if none/ambiguous */
ldbg_status ldbg_graph_color_for_sample_name(const ldbg_graph* g, const char* name, int* color);

/* Iterator<CortexRecord>.next() / getRecord(i) in bulk             CortexGraph.java:183-258
 * records [first, first+n): kmer_words n×W, cov n×C (the reference's signed int view of the
 * LE u32), edges n×C.  Indices >= N yield LDBG_ERR_ARG (the reference returns null, Q2). */
ldbg_status ldbg_graph_records(const ldbg_graph* g, int64_t first, int64_t n,
                               uint64_t* kmer_words, uint32_t* cov, uint8_t* edges);
ldbg_status ldbg_graph_records_dev(const ldbg_graph* g, int64_t first, int64_t n,
                                   uint64_t* d_kmer_words, uint32_t* d_cov, uint8_t* d_edges, void* stream);

/* findRecord(byte[] | CortexByteKmer | CanonicalKmer | String)    CortexGraph.java:272-321
 * Queries are canonicalised on the device (SequenceUtils.alphanumericallyLowestOrientation).
 * idx_out[i] = record index, or -1 where the reference returns null: absent k-mer, non-ACGT
 * query (ASCII form, Q4), or N <= 2 (Q1, cold cache).  cov_out / edges_out (n×C) may be NULL;
 * rows of misses are zero. */
ldbg_status ldbg_graph_find(const ldbg_graph* g, const uint64_t* packed, int64_t n,
                            int64_t* idx_out, uint32_t* cov_out, uint8_t* edges_out);
ldbg_status ldbg_graph_find_ascii(const ldbg_graph* g, const char* kmers, int64_t n,
                                  int64_t* idx_out, uint32_t* cov_out, uint8_t* edges_out);
ldbg_status ldbg_graph_find_dev(const ldbg_graph* g, const uint64_t* d_packed, int64_t n,
                                int64_t* d_idx_out, uint32_t* d_cov_out, uint8_t* d_edges_out, void* stream);

/* ------------------------------------------------------------------ unitigs
 * The compacted graph of a colour set S, built on the device: the unitigs (maximal non-branching paths) that ToGfa1
 * (J/commands/utils/ToGfa1.java:37-145) reads from a FASTA, each in alphanumericallyLowestOrientation (SequenceUtils.java:206-234),
 * numbered in the record order of their first k-mer.  Vertices: records with coverage in a colour of S, both orientations;
 * adjacency: the edge bytes ORed over S, oriented as TraversalUtils.getAllNextKmers / getAllPrevKmers (TraversalUtils.java:510-557)
 * orient them (no quirk Q6).  Not for one rank's part of a hash-sharded table nor its image (LDBG_ERR_UNSUPPORTED); a collection
 * is a graph like any other here.  The graph must stay open while the handle is used. */
typedef struct ldbg_unitigs ldbg_unitigs;
#define LDBG_GFA_PLUS_STRAND 1   /* ldbg_unitigs_write_gfa1: '+' for the positive strand (GFA tools) instead of ToGfa1's ':' */
ldbg_status ldbg_graph_unitigs(const ldbg_graph* g, const int* colors, int n_colors, ldbg_unitigs** out);
/* count, bases of all unitigs together, bases of the longest; build_ms (may be NULL): device time of the build */
ldbg_status ldbg_unitigs_info(const ldbg_unitigs* u, int64_t* count, int64_t* total_bases, int64_t* longest, double* build_ms);
/* ReferenceSequence.getBaseString of FASTA records [first, first+n): offsets[n+1] relative to the first, bases back to back (ASCII,
 * no terminators).  bases == NULL: only the offsets (offsets[n] = bytes needed); too small a capacity: LDBG_ERR_CAPACITY. */
ldbg_status ldbg_unitigs_get(const ldbg_unitigs* u, int64_t first, int64_t n, int64_t* offsets, char* bases, int64_t capacity);
/* the same into device buffers (offsets and bases both on the unitigs' device) */
ldbg_status ldbg_unitigs_get_dev(const ldbg_unitigs* u, int64_t first, int64_t n, int64_t* d_offsets, char* d_bases, int64_t capacity, void* stream);
/* ToGfa1's cov per unitig and colour: the sum of CortexRecord.getCoverage over its k-mers (ToGfa1.java:82-95), n x C, every
 * colour of the graph, wrapping like a Java int */
ldbg_status ldbg_unitigs_coverage(const ldbg_unitigs* u, int64_t first, int64_t n, uint32_t* cov);
/* record -> unitig id, position of its k-mer in the unitig, orientation (1: the unitig holds the reverse complement); -1 for
 * records that are no vertex of S.  Any output may be NULL. */
ldbg_status ldbg_unitigs_of_records(const ldbg_unitigs* u, const int64_t* records, int64_t n, int64_t* unitig, int64_t* position, int8_t* orientation);
/* the unitigs as FASTA: ">id" and the bases on one line each (the input ToGfa1 expects) */
ldbg_status ldbg_unitigs_write_fasta(const ldbg_unitigs* u, const char* path);
/* ToGfa1.execute (ToGfa1.java:37-145) with these unitigs as its FASTA, byte for byte: H, S (RC, AC of sample_color), L in JGraphT
 * edge insertion order.  flags: LDBG_GFA_PLUS_STRAND. */
ldbg_status ldbg_unitigs_write_gfa1(const ldbg_unitigs* u, const char* path, int sample_color, int flags);
ldbg_status ldbg_unitigs_free(ldbg_unitigs* u);

/* ------------------------------------------------------------------ record selection
 * The loop "for (CortexRecord cr : GRAPH) if (test(cr)) cgw.addRecord(...)" of FindROIs (J/commands/discover/roi/FindROIs.java:30-82),
 * FindLowCoverage (J/commands/prefilter/FindLowCoverage.java:32-67), FindDust (FindDust.java:78-135), FindShared (FindShared.java:41-118)
 * and Remove (J/commands/utils/Remove.java:29-86), on the device: the records of a resident table that pass a filter, in record
 * order, and those records packed as a graph.  The filter is a conjunction of clauses, each of which can be switched off; with every
 * clause off it selects every record.  Coverage is compared as CortexRecord.getCoverage returns it (CortexRecord.java:158: the LE u32
 * as a signed int — a stored 0x80000000 is neither == 0 nor > 0, and is < MIN for any MIN). */
typedef struct {
    uint64_t all_zero;      /* every colour of the mask: coverage == 0                          (FindROIs.isNovel :72-82, parents) */
    uint64_t all_positive;  /* every colour of the mask: coverage > 0                           (FindROIs.isNovel, child)          */
    uint64_t any_positive;  /* 0 = off; else at least one colour of the mask has coverage > 0   (FindShared.java:65-71)            */
    uint64_t none_positive; /* every colour of the mask: coverage <= 0 — not one > 0            (Remove.java:50-56)                */
    int32_t  cov_color;     /* -1 = off; else coverage[cov_color] < cov_below                   (FindLowCoverage.java:46)          */
    int32_t  cov_below;
    int32_t  degree_color;  /* -1 = off; else getInDegree + getOutDegree of that colour (CortexRecord.java:287-289: the bits set in
                               its edge byte) > degree_above                                    (FindDust.isDust :133-135)         */
    int32_t  degree_above;
} ldbg_record_filter;
typedef struct ldbg_selection ldbg_selection;
/* The records of g that pass the filter.  Resident tables and collections (of a collection: the view that was opened; Remove iterates
 * the collection, find_view = 0); not one rank's part of a hash-sharded table nor its image (LDBG_ERR_UNSUPPORTED).  A mask bit or a
 * colour at or above the graph's number of colours is LDBG_ERR_ARG.  The graph must stay open while the selection is used. */
ldbg_status ldbg_graph_select(const ldbg_graph* g, const ldbg_record_filter* filter, ldbg_selection** out);
/* FindShared's form: for every record rr of q, cr = g.findRecord(rr.getCanonicalKmer()) (FindShared.java:61-63) and the filter applied
 * to cr; the selection numbers q's records.  A k-mer of q without a record in g — any k-mer when g has two records or fewer (SURVEY
 * Q1) — is LDBG_ERR_NULLPOINTER: the reference dereferences the null (:65-68). */
ldbg_status ldbg_graph_select_lookup(const ldbg_graph* g, const ldbg_record_filter* filter, const ldbg_graph* q, ldbg_selection** out);
ldbg_status ldbg_selection_count(const ldbg_selection* sel, int64_t* n);
/* record numbers [first, first + n) of the selection, ascending (the order of the graph's iterator, CortexGraph.java:183-258) */
ldbg_status ldbg_selection_indices(const ldbg_selection* sel, int64_t first, int64_t n, int64_t* idx);
ldbg_status ldbg_selection_indices_dev(const ldbg_selection* sel, int64_t first, int64_t n, int64_t* d_idx, void* stream);
/* CortexGraphWriter over the selection (J/utils/io/graph/cortex/CortexGraphWriter.java:36-142): every selected record reduced to
 * colours[0..n_colours) in that order (new CortexRecord(cr.getBinaryKmer(), cov, edges, ...), FindROIs.java:55-60, Remove.java:58-72),
 * addRecord, close.  header_path != NULL: setHeader(that graph's header) — as ldbg_ctx_write_records writes it (Q16 and the writer's
 * error-rate constant included); it must have the same k and n_colours colours.  header_path == NULL: the header of
 * FindROIs.makeCortexHeader (:85-105): version 6, the sample names of the projected colours, every other colour field zero / false / "".
 * A selection of no records still writes the header (close() initialises the file, :140-142).  The records are packed on the device
 * and cross the bus once. */
ldbg_status ldbg_selection_write_ctx(const ldbg_selection* sel, const int* colours, int n_colours, const char* header_path, const char* out_path);
/* new CortexGraph(the file ldbg_selection_write_ctx would write) without the file: the packed records stay on the device and are
 * laid out as a resident table there (ldbg_graph_open_device).  Close it with ldbg_graph_close. */
ldbg_status ldbg_selection_open_graph(const ldbg_selection* sel, const int* colours, int n_colours, const char* header_path, ldbg_graph** out);
ldbg_status ldbg_selection_free(ldbg_selection* sel);

/* ------------------------------------------------------------------ RecoverExcludedKmers
 * The loop of J/commands/discover/recover/RecoverExcludedKmers.java:29-108 on the device.  For every record cr of g, in iterator
 * order: coverage[child_colour] > 0 -> written as it is; else, if another colour has coverage > 0: dr = dirty.findRecord(cr's k-mer),
 * and if dr != null && dr.getCoverage(0) > 0 the record is written with coverages[child_colour] = dr.getCoverage(0) (edges unchanged:
 * the reference's edge patch is commented out); every other record is dropped.  Coverage is the Java int in both graphs (a stored
 * 0x80000000 is not > 0), and a dirty of two records or fewer never answers.  *out is an ordinary selection over g — the
 * written records, ascending; count, indices, indices_dev and free work as for any selection — that also holds the child colour's
 * coverage of every written record after the patch.  *n_recovered (optional): numRecordsRecovered.
 * g: whatever ldbg_graph_select accepts.  dirty: a resident single-file table of any number of colours (only colour 0 is read); a
 * collection, one rank's part of a hash-sharded table or its image is LDBG_ERR_UNSUPPORTED.  LDBG_ERR_ARG: child_colour out of range;
 * a dirty of another k-mer size (the reference does not check: a documented divergence).  Both graphs must stay open while the
 * selection is used. */
ldbg_status ldbg_graph_recover(const ldbg_graph* g, int child_colour, const ldbg_graph* dirty, ldbg_selection** out, int64_t* n_recovered);
/* the child colour's coverage after the patch of selected records [first, first + n).  LDBG_ERR_ARG on a selection not made by
 * ldbg_graph_recover (as for the two calls below). */
ldbg_status ldbg_selection_recovered_coverage(const ldbg_selection* sel, int64_t first, int64_t n, int32_t* cov);
/* The reference's file: the header of makeHeader (:98-107: version, k and kmerBits of g, ONE colour whose block is g's block for
 * child_colour, re-serialised as every header written here, Q16 and the writer's error-rate constant included), then per written
 * record what CortexGraphWriter.addRecord writes under a one-colour header (CortexGraphWriter.java:106-138): the k-mer and COLOUR 0's
 * coverage and edge byte.  The patched coverage therefore shows in the file only when child_colour == 0 (the pipeline joins the clean
 * child graph first, so there it is); kept as it is.  No written record still writes the header. */
ldbg_status ldbg_selection_write_recovered(const ldbg_selection* sel, const char* out_path);
/* new CortexGraph(that file) without the file (ldbg_graph_open_device, like ldbg_selection_open_graph).  Close it with ldbg_graph_close. */
ldbg_status ldbg_selection_open_recovered(const ldbg_selection* sel, ldbg_graph** out);

/* ------------------------------------------------------------------ sequences threaded through a graph
 * The inner loop of TrimPartitions (J/commands/discover/call/TrimPartitions.java:35-68), FilterPartitions (:41-140),
 * CountNovelKmersInPartitions (:30-61), Coverage (J/commands/discover/display/Coverage.java:29-47), Call.loadChildWalk
 * (Call.java:2358-2381) and Call.getRegions (:2425-2451): for every window i of every sequence, seq[i:i+k] canonicalised and looked up.
 * Sequence s is bases[offsets[s] .. offsets[s+1]) as given: only upper-case ACGT are bases.  It has max(0, len - k + 1) windows; the
 * windows of all sequences are numbered consecutively.  Per window:
 *   info   bit 0 valid (all k bytes are bases), bit 1 flipped (the reverse complement is the smaller one, by value), bit 2 palindrome,
 *          bit 3 in ROI: the canonical k-mer is a record of `rois` (membership as a HashSet filled by iteration answers it: a `rois` of
 *          one or two records still matches, coverage is not looked at)
 *   rec    the record of the canonical k-mer in `g`; -1 when the window is invalid or absent or g is NULL.  With
 *          LDBG_THREAD_FIND_QUIRK a `g` of two records or fewer answers -1 everywhere, as findRecord does
 *   copy_index (LDBG_THREAD_COPY_INDEX)  earlier windows of the same sequence with the same k-mer string as given (Call.java:2361-2377);
 *          defined for valid windows only: an invalid window gets 0 (the reference counts those among themselves by their bytes)
 * Per sequence: first_hit / last_hit, the smallest / largest in-ROI window relative to the sequence (-1: none); n_hits, its in-ROI
 * windows; n_distinct, the distinct canonical k-mers among them; ends bit 0 / 1: the first / last window is in ROI; and the regions,
 * maximal runs of consecutive in-ROI windows as inclusive (start, stop) pairs in order, as getRegions builds them.
 * LDBG_ERR_ARG: both graphs NULL, graphs that differ in k, an unknown flag, a colour out of range, negative or decreasing offsets.
 * LDBG_ERR_UNSUPPORTED: one rank's part of a hash-sharded table or its image; 2^31 or more windows (counted from the offsets alone,
 * before a byte of `bases` is read).  An empty batch and sequences shorter than k are no errors.  The graphs must stay open while the
 * threading is used. */
typedef struct ldbg_threading ldbg_threading;
enum { LDBG_THREAD_FIND_QUIRK = 1, LDBG_THREAD_COPY_INDEX = 2 };
ldbg_status ldbg_graph_thread(const ldbg_graph* g_or_null, const ldbg_graph* rois_or_null, const char* bases, const int64_t* offsets, int64_t n_seqs,
                              int flags, ldbg_threading** out);
/* the same with the text and the n_seqs + 1 offsets ALREADY IN MEMORY OF THE GRAPHS' DEVICE (the contigs a walk batch left there, a
 * torch tensor's data_ptr): only the offsets come to the host.  stream (a hipStream_t, may be NULL): the stream the work is queued
 * on; work on other streams that produces the inputs must have completed. */
ldbg_status ldbg_graph_thread_dev(const ldbg_graph* g_or_null, const ldbg_graph* rois_or_null, const void* d_bases, const void* d_offsets, int64_t n_seqs,
                                  int flags, void* stream, ldbg_threading** out);
/* device_ms: device time of the kernels of the call that made it.  Any output may be NULL. */
ldbg_status ldbg_threading_info(const ldbg_threading* t, int64_t* n_seqs, int64_t* n_windows, int64_t* n_regions, double* device_ms);
/* windows [first, first + n); any of the three outputs may be NULL, copy_index must be when LDBG_THREAD_COPY_INDEX was not given */
ldbg_status ldbg_threading_windows(const ldbg_threading* t, int64_t first, int64_t n, int64_t* rec, uint8_t* info, int32_t* copy_index);
ldbg_status ldbg_threading_windows_dev(const ldbg_threading* t, int64_t first, int64_t n, void* d_rec, void* d_info, void* d_copy_index, void* stream);
/* getCoverage(colour) of rec as a Java int.  LDBG_ERR_NULLPOINTER when a window of the range has no record (Coverage.java:41-42
 * dereferences the null); cov then still holds the coverages of the windows that have one. */
ldbg_status ldbg_threading_coverage(const ldbg_threading* t, int colour, int64_t first, int64_t n, int32_t* cov);
/* sequences [first_seq, first_seq + n): win_start[n + 1] numbers of their first windows; any output may be NULL */
ldbg_status ldbg_threading_summary(const ldbg_threading* t, int64_t first_seq, int64_t n, int64_t* win_start, int32_t* first_hit, int32_t* last_hit,
                                   int32_t* n_hits, int32_t* n_distinct, uint8_t* ends);
/* region_offsets[n_seqs + 1] into start / stop.  Too small a capacity: LDBG_ERR_CAPACITY, the offsets are filled. */
ldbg_status ldbg_threading_regions(const ldbg_threading* t, int64_t* region_offsets, int32_t* start, int32_t* stop, int64_t capacity);
ldbg_status ldbg_threading_free(ldbg_threading* t);

/* ------------------------------------------------------------------ occurrences of a threading
 * For every record r of the threading's graph: count[r], the windows of t whose rec is r (valid windows only, either strand: the
 * lookup is canonical), and first_window[r], the smallest such window number (-1: none).  rec is taken as the threading has it: under
 * LDBG_THREAD_FIND_QUIRK a graph of two records or fewer has no occurrences.  Both arrays stay on the device.  Stands in for
 * IndexedReference.find(String) (J/utils/io/reference/IndexedReference.java:90-101: the aligner's hits with NM = 0 and a one-element
 * CIGAR, on either strand) where the reference asks "does this k-mer have exactly one place in a reference" (a documented divergence:
 * an exact count, not what an aligner reports).  LDBG_ERR_ARG: a threading made without a graph.  The threading may be freed before
 * the occurrences; the graph must stay open. */
typedef struct ldbg_occurrences ldbg_occurrences;
ldbg_status ldbg_threading_occurrences(const ldbg_threading* t, ldbg_occurrences** out);
/* n_records: the records of the graph; device_ms: device time of the kernel that counted.  Either output may be NULL. */
ldbg_status ldbg_occurrences_info(const ldbg_occurrences* o, int64_t* n_records, double* device_ms);
/* records [first_rec, first_rec + n); either output may be NULL */
ldbg_status ldbg_occurrences_get(const ldbg_occurrences* o, int64_t first_rec, int64_t n, uint32_t* count, int64_t* first_window);
ldbg_status ldbg_occurrences_get_dev(const ldbg_occurrences* o, int64_t first_rec, int64_t n, void* d_count, void* d_first_window, void* stream);
ldbg_status ldbg_occurrences_free(ldbg_occurrences* o);

/* ------------------------------------------------------------------ variant seeds
 * getVariantSeeds of ComputeAssemblyQuality (J/commands/quality/ComputeAssemblyQuality.java:204-286) and of ComputeInheritance
 * (J/commands/inheritance/ComputeInheritance.java:238-322) on the device: the records that pass a filter (S), the string graph over
 * them and their declared neighbours, and the walk along it from every vertex of in-degree 0 and out-degree 1.  The filter is a
 * conjunction; coverage is the Java int (a stored 0x80000000 is neither > 0 nor == 0):
 *   always  isSinglyConnected (:288-299 / :372-383): every colour with coverage > 0 has in-degree 1 and out-degree 1 (the bits set in
 *           either nibble of its edge byte); a record without a covered colour passes
 *   all_zero   every colour of the mask has coverage == 0                     (isUniqueToEval :301-303, the comp colour)
 *   covered[]  mask 0 = off; else the colours of the mask with coverage > 0 number at_least .. at_most; at_least > at_most selects
 *              nothing (isUniqueToEval: {1 << eval, 1, 1}; isSharedWithOnlyOneParent :338-350: {parents, 1, 1}, {drafts, 1, 1};
 *              isSharedWithSomeChildren :352-370: {children, 2, numChildren - 1}, off when numChildren == 1)
 *   unique[]   for every entry whose colour is -1 or has coverage > 0 in the record, the record has exactly one occurrence
 *              (hasUniqueCoordinates :305-309 / :385-404): by `occurrences` made over this same graph (count == 1), or by d_unique, a
 *              caller's byte per record in device memory (non-zero = unique: the door for a host with an aligner).  Exactly one of
 *              the two is set.
 * The string graph has no parallel edges and allows loops.  For r in S with stored k-mer F and reverse complement R (one vertex for
 * an even-k palindrome) and every covered colour c: for every in-edge base b of c, P = b + F[:-1] and the edges P -> F, R -> rc(P); for
 * every out-edge base b, N = F[1:] + b and the edges F -> N, rc(N) -> R (CortexRecord.java:214-285: A C G T in bit order).  Whether a
 * neighbour is in S is decided by value, not by findRecord: a table of one or two records behaves like any other.  From every vertex
 * of in-degree 0 and out-degree 1 the single successor is followed while the current vertex has out-degree 1, up to a vertex that is
 * on the chain already (ComputeAssemblyQuality's guard :261-274; ComputeInheritance has none and never returns there: both get the
 * guarded result); a chain of more than 3 vertices makes canonical(chain[1]) a good seed.
 * *out: an ordinary selection over g holding the good seeds, ascending (count, indices, indices_dev, write_ctx, open_graph, free).
 * counts (optional): as the reference logs them.
 * g: a resident single-file table.  LDBG_ERR_UNSUPPORTED: a collection (ComputeAssemblyQuality joins first), one rank's part of a
 * hash-sharded table or its image.  LDBG_ERR_ARG: a NULL filter, a mask bit or colour at or above the graph's number of colours,
 * n_covered / n_unique beyond the arrays, an entry with neither or both inputs, occurrences made over another graph.  An empty S is
 * no error.  The graph must stay open while the selection is used. */
#define LDBG_SEED_MAX_COVERED 3
#define LDBG_SEED_MAX_UNIQUE 8
typedef struct { uint64_t mask; int32_t at_least, at_most; } ldbg_seed_covered;
typedef struct { int32_t colour; const ldbg_occurrences* occurrences; const void* d_unique; } ldbg_seed_unique;
typedef struct {
    uint64_t all_zero;
    int32_t n_covered;
    ldbg_seed_covered covered[LDBG_SEED_MAX_COVERED];
    int32_t n_unique;
    ldbg_seed_unique unique[LDBG_SEED_MAX_UNIQUE];
} ldbg_seed_filter;
typedef struct {
    int64_t n_seeds;     /* |S|: "seed kmers for putative variants"                  */
    int64_t n_unique;    /* distinct vertices of in-degree 0 and out-degree 1        */
    int64_t n_good;      /* good seeds: the selection's count                        */
    double device_ms;    /* device time of the kernels of the call                   */
} ldbg_seed_counts;
ldbg_status ldbg_graph_variant_seeds(const ldbg_graph* g, const ldbg_seed_filter* filter, ldbg_selection** out, ldbg_seed_counts* counts);

/* ------------------------------------------------------------------ hash partitioning over devices
 * owner[i] = mix64(minimizer of canonical k-mer i) mod world — the rule by which the sorted table is split into per-device
 * shards (each still sorted) and by which a lookup is routed to the shard that can answer it.  The minimizer is the m-mer, m = (k + 2) / 3
 * (k itself up to k = 8), taken in its own canonical orientation, whose mixed value is smallest: a k-mer and its reverse complement
 * agree, and a run of consecutive k-mers of a walk shares it — their rows live on one shard and travel together (ldbg_image_serve_chain).  The _dev form
 * works on device buffers (d_canon, n x W canonical words, may be NULL) and is what the exchange step of
 * corticall_amd/distributed.py calls between its all-to-alls; the host form is used when the shards are cut. */
ldbg_status ldbg_shard_owner_dev(int k, const uint64_t* d_packed, int64_t n, int world, uint64_t* d_canon, int32_t* d_owner, void* stream);
ldbg_status ldbg_shard_owner(int k, const uint64_t* packed, int64_t n, int world, int device, int32_t* owner);

/* The GLOBAL neighbour index of a shard (corticall_amd/csrc/shard.cpp): for each record and each of its 8 possible neighbours the
 * owner, the record number in the owner's shard and the orientation — one routed findRecord per edge, memoised at load.
 * All buffers are device buffers of the calling rank; calls return when the work is done. */
ldbg_status ldbg_shard_nbr_queries(const ldbg_graph* shard, int64_t first, int64_t n, uint64_t* d_words /* [8n][W] */, uint8_t* d_flips /* [8n] */,
                                   uint8_t* d_have /* [8n] 0 = no colour carries that edge: no query */);
ldbg_status ldbg_shard_set_nbr(ldbg_graph* shard, int64_t first, int64_t n, const int32_t* d_owner, const int64_t* d_local_idx, const uint8_t* d_flips);

/* Traversals over the hash-sharded table: the local IMAGE (corticall_amd/csrc/image.h).
 * A walk lives on the rank that was given its seed (visited set, link store, path, stopping rule never move).  The rank keeps an
 * image — the rows it has been sent so far, laid out like a shard's probe table, with the neighbour index rewritten to image
 * slots — and the unchanged traversal kernels run on it: link-guided steps, junction choices, every quirk, even k.  A strand that
 * is about to read a row that is not there suspends and files a request.  One bulk-synchronous round =
 *   ldbg_engine_sharded_walk_round   every strand runs until it suspends or ends
 *   ldbg_image_bucket                requests -> one block per owner  [world][cap] of global id keys
 *   (all-to-all)                     RCCL over xGMI: torch.distributed in corticall_amd/distributed.py
 *   ldbg_image_serve                 the owners write the rows asked for: global id key | 8 global neighbour ids | probe row
 *   (all-to-all)
 *   ldbg_image_insert                arrivals enter the image; rows fetched for one strand serve all strands of the rank
 * `stream`: a HIP stream (e.g. torch's current stream) all calls of a round are queued on — none of them synchronises with the
 * host; NULL = the library's own stream.  A global id key is  (record number in the owner's shard + 1) | owner << 40. */
typedef struct ldbg_image ldbg_image;
struct ldbg_engine;
ldbg_status ldbg_image_create(const ldbg_graph* shard_with_neighbour_index, int64_t capacity_rows, int64_t global_records, ldbg_image** out);
ldbg_status ldbg_image_destroy(ldbg_image* im);
/* the image as a graph handle: engines over the sharded table are created on it (owned by the image; do not close it) */
ldbg_status ldbg_image_graph(ldbg_image* im, ldbg_graph** image_graph);
ldbg_status ldbg_image_row_bytes(const ldbg_image* im, int* bytes);
ldbg_status ldbg_image_clear(ldbg_image* im);
ldbg_status ldbg_image_request(ldbg_image* im, const uint64_t* d_keys, int64_t n, void* stream);      /* explicit requests: seeds, sinks */
ldbg_status ldbg_image_reset_requests(ldbg_image* im, void* stream);
ldbg_status ldbg_image_bucket(ldbg_image* im, int world, uint32_t cap_per_owner, uint64_t* d_send /* [world][cap_per_owner], 0 = unused */, void* stream);
ldbg_status ldbg_image_serve(const ldbg_image* im, int my_rank, const uint64_t* d_keys, int64_t n, uint8_t* d_rows_out, void* stream);
/* as ldbg_image_serve, `depth` row slots per request: the row asked for, then rows around it that this owner holds too (its unique
 * neighbours outwards in both directions; ownership goes by minimizer, so these are mostly the rows the asker wants next).  A slot
 * whose key is 0 is unused.  d_rows_out: [n][depth][row_bytes]; hand all n * depth slots to ldbg_image_insert. */
ldbg_status ldbg_image_serve_chain(const ldbg_image* im, int my_rank, const uint64_t* d_keys, int64_t n, int depth, uint8_t* d_rows_out, void* stream);
ldbg_status ldbg_image_insert(ldbg_image* im, const struct ldbg_engine* engine_or_null, const uint8_t* d_rows, int64_t n, void* stream);
ldbg_status ldbg_image_lookup(const ldbg_image* im, const uint64_t* d_keys, int64_t n, int32_t* d_slots /* -1 = not in the image */, void* stream);
ldbg_status ldbg_image_counters(const ldbg_image* im, int64_t* n_rows, int64_t* n_requests, int* overflow);   /* synchronises */
/* TraversalEngine.walk over the image (ContigStopper; links bound to the shard graph).  begin: seeds (n x k ASCII, host) with the
 * image slots of their records (device, -1 = none; their rows are already in the image); round: d_stats (device, 3 x int64) =
 * {strands of this rank not done yet, requests filed, the image is full}; finish: results as after ldbg_engine_walk_batch_run.
 * A full image never fills a request again: when the third value is set on any rank, every rank stops its rounds, enlarges its
 * image and runs the batch again (begin drops a batch that was not finished). */
ldbg_status ldbg_engine_sharded_walk_begin(struct ldbg_engine* e, ldbg_image* im, const char* seeds, int64_t n, const int32_t* d_seed_slot, void* stream);
ldbg_status ldbg_engine_sharded_walk_round(struct ldbg_engine* e, int64_t* d_stats);
ldbg_status ldbg_engine_sharded_walk_finish(struct ldbg_engine* e, int64_t* total_contig_bytes, int64_t* kmers_traversed);
/* TraversalEngine.dfs(source, sinks...) over the image, any stopping rule that does not consult a ROI graph.  The library runs the
 * rounds and calls round_done(user) after each: the caller makes the round's exchange there (bucket, all-to-all, serve, all-to-all,
 * insert) and returns 1 once no rank has a search in progress, 2 to give the batch up on every rank (d_stats as above: a full image;
 * the call then fails with LDBG_ERR_CAPACITY "IMAGE_FULL"), 0 otherwise.  d_seed_slot / d_sink_slot: image slots of the
 * sources' and sinks' records (-1 = none), their rows already in the image.  Capacity errors ("LINKSTORE_FULL", "LOG_FULL",
 * "DEPTH_OVERFLOW") enlarge the engine's stores: run the batch again on every rank.  Result: as ldbg_engine_dfs_batch; `rec` of a
 * vertex is its image slot (>= 0: the vertex has a record). */
struct ldbg_dfs_result;
ldbg_status ldbg_engine_sharded_dfs_batch(struct ldbg_engine* e, ldbg_image* im, const char* sources, int64_t n, const char* sinks, const int64_t* sink_offsets,
                                          const int32_t* d_seed_slot, const int32_t* d_sink_slot, int (*round_done)(void* user), void* user,
                                          int64_t* d_stats, void* stream, struct ldbg_dfs_result** out);

/* ------------------------------------------------------------------ links: L3-L4
 * new CortexLinks(path) -> CortexLinksMap        J/utils/io/graph/links/CortexLinks.java:16-25,
 * CortexLinksIterable.java:49-226 (.ctp.gz text, JSON header v2/3/4).  Bound to a graph for k / device. */
ldbg_status ldbg_links_open(const char* path, const ldbg_graph* g, ldbg_links** out);
ldbg_status ldbg_links_close(ldbg_links* l);
/* ------------------------------------------------------------------ links construction
 * TempLinksAssembler.buildLinks (J/utils/assembler/TempLinksAssembler.java:29): the link annotations that the reads of one sample
 * leave on an open graph, built on the device.  Reads are passed as ldbg_build_sample passes sequences: read i is
 * bases[offsets[i], offsets[i + 1]), n_reads + 1 offsets, not decreasing.  Each read is threaded as given and reverse-complemented,
 * and is NOT upper-cased.  In the string graph of the sample's colour (both orientations of every record with coverage there, and
 * every k-mer an edge of that colour names) a link starts at every k-mer followed by one of in-degree above 1 and records the base
 * taken at every later fork (a k-mer of out-degree above 1 followed by a k-mer of the graph); links = CortexJunctionsRecords of
 * coverage 1, filed in a set under the canonical k-mer.  The orientation of a k-mer is decided by value.
 * LDBG_ERR_CORTEXJDK: an unknown sample; a window of a read of k + 1 bytes or more that is no k-mer of that string graph, a window
 * holding a byte other than ACGT included (the reference's graph library throws).  A read shorter than k + 1 adds nothing.
 * LDBG_ERR_ARG: flags other than 0, a null pointer, negative or decreasing offsets.  LDBG_ERR_UNSUPPORTED: 2^31 or more windows,
 * links or junction bytes (the sum of the links' lengths) in one call; one rank's part of a hash-sharded table, its image, a
 * collection.  Nothing is written and no handle returned on an error.
 * The file: ctp version 4, the text byte for byte what TempLinksAssembler writes (gzip container apart): its JSON header, its
 * HashMap order of k-mers and HashSet order of junction records.  num_kmers_with_links / num_links may be NULL. */
ldbg_status ldbg_links_build_ctp(const ldbg_graph* g, const char* sample_name, const char* bases, const int64_t* offsets, int64_t n_reads, int flags,
                                 const char* out_path, int64_t* num_kmers_with_links, int64_t* num_links);
/* the same link set bound to the graph without a file: in every respect the handle ldbg_links_open returns for that file */
ldbg_status ldbg_links_build(const ldbg_graph* g, const char* sample_name, const char* bases, const int64_t* offsets, int64_t n_reads, int flags,
                             ldbg_links** out);
/* IndexLinks: J/commands/index/links/IndexLinks.java:62-135.  The records of a link file (.ctp / .ctp.gz, v2-4) re-written as a BGZF file
 * (out_path, conventionally .ctp.bgz) with the big-endian LNKIDX index beside it (out_path + ".idx": per record the BGZF virtual offset
 * and the text length, ordered by k-mer string).  ldbg_links_open on out_path then reads every record through that index, as
 * CortexLinksRandomAccess does (CortexLinksRandomAccess.java:33-118), with that back-end's record semantics. */
ldbg_status ldbg_links_index(const char* in_path, const char* out_path, const char* source, int64_t* num_records);
ldbg_status ldbg_links_source(const ldbg_links* l, char* buf, int buflen);       /* ConnectivityAnnotations.getSource() */
ldbg_status ldbg_links_info(const ldbg_links* l, int* version, int* num_colors, int* k,
                            int64_t* num_kmers_in_graph, int64_t* num_kmers_with_links, int64_t* num_links);
ldbg_status ldbg_links_sample_name(const ldbg_links* l, int color, char* buf, int buflen);
/* ConnectivityAnnotations.containsKey / get     J/utils/io/graph/ConnectivityAnnotations.java:23-25
 * Writes the record as text "KMER n\n(F|R) len cov[,cov] junctions\n..." in the reference's HashSet
 * iteration order; *found = 0 and empty text when the k-mer has no links. */
ldbg_status ldbg_links_get(const ldbg_links* l, const char* kmer_ascii, int* found, char* buf, int64_t buflen);

/* ------------------------------------------------------------------ engine: C1, E1-E3, D1-D2, W1, S1-S3 */
typedef enum {   /* J/utils/stoppingrules/ (one enumerator per rule class) */
    LDBG_STOP_CONTIG = 0, LDBG_STOP_CYCLE_COLLAPSING_CONTIG, LDBG_STOP_DESTINATION, LDBG_STOP_EXPLORATION,
    LDBG_STOP_NOVEL_PARTITION, LDBG_STOP_NOVEL_KMER_LIMITED_CONTIG, LDBG_STOP_NOVEL_CONTINUATION,
    LDBG_STOP_BUBBLE_CLOSING, LDBG_STOP_BUBBLE_OPENING, LDBG_STOP_CONTAMINANT, LDBG_STOP_DUST,
    LDBG_STOP_GAP_CLOSING, LDBG_STOP_NAHR, LDBG_STOP_NOVEL_KMER_AGGREGATION, LDBG_STOP_ORPHAN,
    LDBG_STOP_PAIRED_READ_CLOSING, LDBG_STOP_TIP_BEGINNING, LDBG_STOP_TIP_END, LDBG_STOP_VISUALIZATION,
    LDBG_STOP_COUNT
} ldbg_stopper;
enum { LDBG_DIR_BOTH = 0, LDBG_DIR_FORWARD = 1, LDBG_DIR_REVERSE = 2 };   /* TraversalDirection */
enum { LDBG_OP_OR = 0, LDBG_OP_AND = 1 };                                 /* GraphCombinationOperator */
#define LDBG_MAX_COLORS 32

/* TraversalEngineConfiguration (J/utils/traversal/TraversalEngineConfiguration.java:19-37) as a POD;
 * ldbg_engine_config_default() fills the reference's defaults (BOTH, OR, ContigStopper, 75000). */
typedef struct {
    const ldbg_graph* graph;
    const ldbg_graph* rois;                 /* may be NULL */
    const ldbg_links* const* links;         /* nlinks entries; order = order of addition */
    int nlinks;
    int traversal_colors[LDBG_MAX_COLORS]; int n_traversal;      /* LinkedHashSet: insertion order */
    int joining_colors[LDBG_MAX_COLORS]; int n_joining;          /* TreeSet */
    int recruitment_colors[LDBG_MAX_COLORS]; int n_recruitment;  /* TreeSet */
    int secondary_colors[LDBG_MAX_COLORS]; int n_secondary;      /* TreeSet */
    int direction;                          /* LDBG_DIR_* */
    int combination_operator;               /* LDBG_OP_* */
    int stopping_rule;                      /* ldbg_stopper */
    int max_branch_length;                  /* maxLength, default 75000 */
    int connect_all_neighbors;
    int strict_java_flip;                   /* 1: CanonicalKmer.isFlipped by Arrays.hashCode inequality (Q6) */
} ldbg_engine_config;
void ldbg_engine_config_default(ldbg_engine_config* cfg);

/* TraversalEngineFactory.make()                 J/utils/traversal/TraversalEngineFactory.java:54-88
 * Threads: an engine is used by one host thread at a time (as a TraversalEngine object is in the reference: it holds the cursor's
 * state).  DIFFERENT engines — on one graph or on several — may be used from different host threads at the same time: every engine
 * over a resident table queues its work on a HIP stream of its own, and batches of two engines overlap on the device. */
ldbg_status ldbg_engine_create(const ldbg_engine_config* cfg, ldbg_engine** out);
ldbg_status ldbg_engine_destroy(ldbg_engine* e);

/* walk(seed) + TraversalUtils.toContig, for n seeds at once       TraversalEngine.java:108-110,
 * TraversalUtils.java:367-488.  seeds: n × k ASCII.  The contigs are written back to back into
 * contig_arena (ASCII); offsets[n+1]; walk_len[i] = number of vertices of walk i (0: empty walk,
 * empty contig).  kmers_traversed (may be NULL) receives the number of dfs loop iterations
 * (TraversalEngine.java:373: one per vertex a branch stands on) the batch performed (SURVEY §8d's unit).  If the arena is too small, LDBG_ERR_CAPACITY is
 * returned and offsets[n] holds the required size. */
ldbg_status ldbg_engine_walk_batch(ldbg_engine* e, const char* seeds, int64_t n,
                                   char* contig_arena, int64_t arena_capacity, int64_t* offsets,
                                   int64_t* walk_len, int64_t* kmers_traversed);
/* two-phase device form: run the batch (results stay in HBM), then query sizes / copy out */
ldbg_status ldbg_engine_walk_batch_run(ldbg_engine* e, const char* seeds, int64_t n,
                                       int64_t* total_contig_bytes, int64_t* kmers_traversed);
ldbg_status ldbg_engine_walk_batch_fetch(ldbg_engine* e, char* contig_arena, int64_t arena_capacity,
                                         int64_t* offsets, int64_t* walk_len);
/* the same batch with the seeds ALREADY IN DEVICE MEMORY (d_seeds: n x k ASCII bytes on the engine's device, e.g. the output of a seed
 * selection that ran there, or a torch uint8 CUDA tensor's data_ptr): nothing crosses the bus before the walks start.  The seeds must
 * stay valid until the call returns; work queued on other streams that produces them must have completed (the call does not wait
 * for foreign streams).  Results as after ldbg_engine_walk_batch_run. */
ldbg_status ldbg_engine_walk_batch_run_device(ldbg_engine* e, const void* d_seeds, int64_t n,
                                              int64_t* total_contig_bytes, int64_t* kmers_traversed);
/* Page-locked host memory for result arenas (contig_arena above): a download into it runs at the bus rate (C3: 780 MB of contigs in
 * about 16 ms); into ordinary memory the library stages the copy through its own page-locked buffers (about twice as long).  A JNI
 * host wraps the block in a direct ByteBuffer (NewDirectByteBuffer) and reads the contigs in place. */
ldbg_status ldbg_host_alloc(int64_t bytes, void** out);
ldbg_status ldbg_host_free(void* p);
/* vertices of walk i of the last batch: packed k-mer words (len × W), record index (-1 = null
 * CortexRecord), copyIndex, index (CortexVertex.java:20-35) */
ldbg_status ldbg_engine_walk_vertices(ldbg_engine* e, int64_t walk, int64_t capacity, int64_t* len,
                                      uint64_t* kmer_words, int64_t* rec, int32_t* copy_index, int32_t* index);

/* Which ROI k-mers the walks of the last batch pass through (the engine must have been made with a ROI graph):
 * what Partition.markUsedRois needs (J/commands/discover/call/Partition.java:238-257).  offsets[n+1] into hits (numbers
 * of ROI records; order within a walk is arbitrary; empty walks have none); has_null[i] != 0: the dfs graph of seed i
 * holds a vertex without a record (the reference's bookkeeping throws NullPointerException on those).  If hits is too
 * small, LDBG_ERR_CAPACITY is returned and offsets[n] holds the required number. */
ldbg_status ldbg_engine_walk_roi_hits(ldbg_engine* e, int64_t* offsets, uint32_t* hits, int64_t capacity, uint8_t* has_null);

/* dfs(source, sinks...) for n sources                               TraversalEngine.java:64-106, 356-482
 * sources n × k ASCII; sinks as CSR over ASCII k-mers (sink_offsets[n+1] counts k-mers; may be NULL). */
ldbg_status ldbg_engine_dfs_batch(ldbg_engine* e, const char* sources, int64_t n,
                                  const char* sinks, const int64_t* sink_offsets, ldbg_dfs_result** out);
/* result i: is_null = dfs returned null; vertices in insertion order; edges (src,dst index into vertices, colour).
 * The graphs (record numbers, copy indices, indices, edges) are complete when dfs_batch returns; the k-mer words of the
 * vertices are gathered from the device the first time they are asked for (kmer_words != NULL, or _walk), so the graph
 * handle must still be open then. */
ldbg_status ldbg_dfs_result_sizes(const ldbg_dfs_result* r, int64_t i, int* is_null, int64_t* n_vertices, int64_t* n_edges);
ldbg_status ldbg_dfs_result_get(const ldbg_dfs_result* r, int64_t i,
                                uint64_t* kmer_words, int64_t* rec, int32_t* copy_index, int32_t* index,
                                int32_t* edge_src, int32_t* edge_dst, int32_t* edge_color);
/* TraversalUtils.toWalk(g, seed, colour) + toContig on result i    TraversalUtils.java:367-488 */
ldbg_status ldbg_dfs_result_walk(const ldbg_dfs_result* r, int64_t i, const char* seed, int color,
                                 char* contig, int64_t capacity, int64_t* len);
/* dfs(Collection<String> sources, Collection<String> sinks)            TraversalEngine.java:37-62
 * = ldbg_engine_dfs_batch with every source given all the sinks, then this: the graphs of results which[0..m) of `r` that are not null,
 * merged in that order — the first as it is, each further one with Graphs.addGraph (vertices the merged graph does not hold yet; edges
 * refused when an equal CortexEdge is present).  *out is a result with ONE graph (index 0; null when every source returned null). */
ldbg_status ldbg_dfs_result_merge(struct ldbg_dfs_result* r, const int64_t* which, int64_t m, struct ldbg_dfs_result** out);
ldbg_status ldbg_dfs_result_free(ldbg_dfs_result* r);
ldbg_status ldbg_engine_dfs_kmers_traversed(const ldbg_engine* e, int64_t* n);

/* cursor: seek / next / previous / hasNext / hasPrevious          TraversalEngine.java:241-339
 * (stateful, batch of one; each call runs on the device) */
/* getNextVertices / getPrevVertices of n k-mers (n x k ASCII)            TraversalEngine.java:147-239
 * as CSR: offsets[n+1]; vertex j: packed k-mer words kmer_words[j*W .. ], rec[j] (record index, -1 = null CortexRecord).  The vertices of
 * one query come in the iteration order of the HashSet<CortexVertex> the reference returns.  capacity: vertices the arrays hold (4 n is
 * always enough).  A k-mer without a record has no neighbours — NullPointerException (Q14) when recruitment colours are configured. */
ldbg_status ldbg_engine_neighbours_batch(struct ldbg_engine* e, const char* kmers, int64_t n, int forward, int64_t* offsets,
                                         uint64_t* kmer_words, int64_t* rec, int64_t capacity);
/* assemble(seed)                                                        TraversalEngine.java:112-145
 * seek(seed), next() while hasNext() and fewer than maxBranchLength vertices; the same with previous(); result in contig order:
 * the previous() vertices (last one first), the seed's own vertex, the next() vertices.  *len = vertices; LDBG_ERR_CAPACITY with *len set
 * when the arrays are too small (call with capacity 0 to learn the length). */
ldbg_status ldbg_engine_assemble(struct ldbg_engine* e, const char* seed, int64_t capacity, int64_t* len, uint64_t* kmer_words, int64_t* rec);
ldbg_status ldbg_engine_seek(ldbg_engine* e, const char* kmer);
ldbg_status ldbg_engine_has_next(ldbg_engine* e, int* yes);
ldbg_status ldbg_engine_has_previous(ldbg_engine* e, int* yes);
ldbg_status ldbg_engine_next(ldbg_engine* e, char* kmer_out, int64_t* rec_out);
ldbg_status ldbg_engine_previous(ldbg_engine* e, char* kmer_out, int64_t* rec_out);

/* n cursors advanced to their end in one call                           TraversalEngine.java:112-145, 241-339
 * Per seed (n x k ASCII) exactly the reference's loops over its cursor: direction LDBG_DIR_FORWARD / _REVERSE is assemble(seed, goForward)
 * (:128-145: seek(seed), then next() / previous() while hasNext() / hasPrevious() and fewer than max_steps vertices are collected; the
 * seed's own vertex is not part of the result; reverse results come in contig order, the last one stepped onto first); LDBG_DIR_BOTH is
 * assemble(seed) (:112-126): the reverse part, the seed's vertex (its record may be -1), the forward part.  Each direction starts from a
 * seek of its own.  max_steps <= 0: the engine's maxBranchLength; more than 2^20: LDBG_ERR_ARG.  A seed that is no k-mer over ACGT
 * (lower case included) has no record and no neighbour; its vertex comes back with all-zero words.
 *
 * stop (may be NULL) is tested after every step on the vertex just stepped onto; a stopping vertex is part of the result (the loops of
 * ComputeInheritance.callVariant :119-165 and ComputeAssemblyQuality.callVariant :104-149 add it and then break):
 *   colour >= 0           stop when the vertex's record has coverage > 0 (as a Java int) in that colour.  A vertex without a record is
 *                         the reference's NullPointerException: the seed gets LDBG_CURSOR_NULLPOINTER, its direction ends with that vertex.
 *   arrival_degree_one    additionally the record's degree in that colour must be exactly 1 on the side the walk arrives from: going
 *                         forward the in-degree when the k-mer stepped onto equals the record's k-mer and the out-degree when it is the
 *                         reverse complement, going back the mirror (ComputeAssemblyQuality.java:114,126; compared by value).
 *   targets               n x k ASCII or NULL; stop when the k-mer stepped onto equals the seed's target as a string.  An entry that is
 *                         no k-mer over ACGT means "none for this seed".  (With links bound CortexVertex.equals also compares the
 *                         vertices' sources; that part is not pinned by any vector and is not compared here.)
 * Order within a step, as in the reference: step, add, stop test, then the loop condition; when both parts of the condition fail the
 * end reason is LDBG_CURSOR_END.  One failing seed does not fail the call, and the bytes of a result depend on the inputs alone.
 * LDBG_ERR_UNSUPPORTED: an engine over one rank's part of a hash-sharded table or its image.  LDBG_ERR_ARG: n < 0, a colour at or above
 * the graph's number of colours, an unknown direction, max_steps above 2^20, a null pointer with n > 0.  n == 0: an empty result.
 * The _device form takes the seeds (and stop->targets) where they are in this engine's device memory, as the walk's _run_device form. */
typedef struct ldbg_cursor_result ldbg_cursor_result;
typedef struct {
    int colour;                 /* -1: no colour rule */
    int arrival_degree_one;
    const char* targets;
} ldbg_cursor_stop;
enum { LDBG_CURSOR_END = 0,     /* no single next vertex */
       LDBG_CURSOR_LIMIT = 1,   /* max_steps vertices collected */
       LDBG_CURSOR_STOP = 2,    /* the colour rule or the target fired */
       LDBG_CURSOR_FAILED = 3   /* the direction ended in the seed's status */ };
enum { LDBG_CURSOR_OK = 0,
       LDBG_CURSOR_NULLPOINTER = 1,   /* where ldbg_engine_assemble returns LDBG_ERR_NULLPOINTER, and a missing record under a colour rule */
       LDBG_CURSOR_CAPACITY = 2       /* the cursor's link store is full */ };
ldbg_status ldbg_engine_cursor_batch(ldbg_engine* e, const char* seeds, int64_t n, int direction, int64_t max_steps,
                                     const ldbg_cursor_stop* stop, ldbg_cursor_result** out);
ldbg_status ldbg_engine_cursor_batch_device(ldbg_engine* e, const void* d_seeds, int64_t n, int direction, int64_t max_steps,
                                            const ldbg_cursor_stop* stop, ldbg_cursor_result** out);
/* seeds and vertices of a result; words per k-mer */
ldbg_status ldbg_cursor_result_sizes(const ldbg_cursor_result* r, int64_t* n_seeds, int64_t* n_vertices, int* kmer_words);
/* offsets[n + 1] (CSR over the vertices, in seed order); per vertex the packed k-mer as stepped onto (kmer_words[j * W ..]) and rec[j]
 * (-1: no record); per seed n_reverse, n_forward, seed_rec (findRecord(seed), -1: none), the end reason of each direction
 * (LDBG_CURSOR_END for a direction that was not asked for) and the status.  Any pointer may be NULL.  The _dev form copies into device
 * memory on `stream` (NULL: the default stream) and returns without waiting for it. */
ldbg_status ldbg_cursor_result_get(const ldbg_cursor_result* r, int64_t* offsets, uint64_t* kmer_words, int64_t* rec, int32_t* n_reverse,
                                   int32_t* n_forward, int64_t* seed_rec, uint8_t* end_reverse, uint8_t* end_forward, uint8_t* status);
ldbg_status ldbg_cursor_result_get_dev(const ldbg_cursor_result* r, void* d_offsets, void* d_kmer_words, void* d_rec, void* d_n_reverse,
                                       void* d_n_forward, void* d_seed_rec, void* d_end_reverse, void* d_end_forward, void* d_status,
                                       void* stream);
ldbg_status ldbg_cursor_result_free(ldbg_cursor_result* r);

/* callVariant of n seeds in one call              J/commands/inheritance/ComputeInheritance.java:102-236, trimToAlleles :406-433,
 * toContig J/utils/traversal/TraversalUtils.java:367-381.  The per-seed reading: child_engine traverses the child's
 * colour alone, parent_engine the colour of the parent that does not share the child's allele (stop_colour); both are engines over the
 * same graph without links or recruitment colours.  Per seed (n x k ASCII):
 *   1. the child contig: assemble(seed) on child_engine with the stop rule "coverage > 0 in stop_colour" in both directions (:119-145);
 *      source = its first vertex when the reverse direction ended on the rule, destination = its last when the forward one did;
 *   2. the parent contig: on parent_engine seek(source as stepped), next() until the k-mer stepped onto equals the destination as a
 *      string (:155-164): the source, then those vertices;
 *   3. per colour of sum_mask (bit c = colour c, ascending) the exact sum of getCoverage (the Java int) over the child contig, and the sum
 *      in stop_colour over the parent contig, each with a flag set where the sum of |coverage| is 2^24 or more (the reference adds in
 *      float, :170-174, :202-206: below that the float sum is this integer; a flagged sum is redone by the caller in float, in order);
 *   4. st, s0end, s1end of trimToAlleles(toContig(child contig), toContig(parent contig)) and the two alleles' text.
 * Status per seed; the first that applies, in this order: a status of the first batch (NULLPOINTER, CAPACITY); LIMIT when a direction of
 * it collected max_steps vertices (the reference's loops have no limit: such a seed is reported, not called); NO_SOURCE; NO_DESTINATION;
 * a status of the third batch, a vertex without a record on the parent contig included (NULLPOINTER: :172 dereferences it); LIMIT;
 * NOT_REACHED; CALLED.  Sums, st, s0end, s1end and alleles are those of CALLED seeds and zero / empty for every other; n_child and
 * source_rec / dest_rec (-1: none) are filled for every seed, n_parent (the source included) for seeds with both.
 * max_steps as ldbg_engine_cursor_batch, for every batch.  One failing seed does not fail the call, and the bytes of a result depend on
 * the inputs alone.  LDBG_ERR_UNSUPPORTED: an engine over one rank's part of a hash-sharded table or its image.  LDBG_ERR_ARG: n < 0,
 * stop_colour negative or at or above the graph's number of colours, a bit of sum_mask at or above it, engines over different graphs,
 * an engine with links or recruitment colours bound, max_steps above 2^20, a null pointer.  n == 0: an empty result.
 * The _device form takes the seeds where they are in the engines' device memory. */
typedef struct ldbg_variant_result ldbg_variant_result;
enum { LDBG_VARIANT_CALLED = 0,
       LDBG_VARIANT_NO_SOURCE = 1,        /* the reverse direction ended without the rule firing */
       LDBG_VARIANT_NO_DESTINATION = 2,   /* the forward direction did */
       LDBG_VARIANT_NOT_REACHED = 3,      /* the parent's cursor ended before the destination */
       LDBG_VARIANT_NULLPOINTER = 4,      /* LDBG_CURSOR_NULLPOINTER of either batch */
       LDBG_VARIANT_CAPACITY = 5,         /* LDBG_CURSOR_CAPACITY of either batch */
       LDBG_VARIANT_LIMIT = 6             /* a direction ended on LDBG_CURSOR_LIMIT */ };
/* where ldbg_variant_result_get writes; any pointer may be NULL.  n seeds, m colours in sum_mask, W words per k-mer. */
typedef struct {
    uint8_t* status;             /* [n] LDBG_VARIANT_* */
    int64_t* source_rec;         /* [n] */
    int64_t* dest_rec;           /* [n] */
    int32_t* n_child;            /* [n] vertices of the child contig */
    int32_t* n_parent;           /* [n] vertices of the parent contig, the source included */
    int32_t* st;                 /* [n] */
    int32_t* s0end;              /* [n] */
    int32_t* s1end;              /* [n] */
    int64_t* child_sum;          /* [n][m] */
    uint8_t* child_flag;         /* [n][m] */
    int64_t* parent_sum;         /* [n] */
    uint8_t* parent_flag;        /* [n] */
    int64_t* allele_offsets;     /* [2n + 1]: the child's allele of seed i is alleles[offsets[2i] .. offsets[2i + 1]), the parent's the next */
    char* alleles;               /* [allele_bytes] ASCII */
    /* the contigs, as CSR over packed k-mers (as stepped onto) and records: the child's whole; the parent's vertices AFTER the source
     * (the source is the child contig's first vertex), empty for a seed without both ends */
    int64_t* child_offsets;      /* [n + 1] */
    uint64_t* child_words;       /* [n_child_vertices][W] */
    int64_t* child_rec;          /* [n_child_vertices] */
    int64_t* parent_offsets;     /* [n + 1] */
    uint64_t* parent_words;      /* [n_parent_vertices][W] */
    int64_t* parent_rec;         /* [n_parent_vertices] */
} ldbg_variant_arrays;
ldbg_status ldbg_engine_variant_batch(ldbg_engine* child_engine, ldbg_engine* parent_engine, const char* seeds, int64_t n, int stop_colour,
                                      int64_t max_steps, uint64_t sum_mask, ldbg_variant_result** out);
ldbg_status ldbg_engine_variant_batch_device(ldbg_engine* child_engine, ldbg_engine* parent_engine, const void* d_seeds, int64_t n,
                                             int stop_colour, int64_t max_steps, uint64_t sum_mask, ldbg_variant_result** out);
ldbg_status ldbg_variant_result_sizes(const ldbg_variant_result* r, int64_t* n_seeds, int* n_colours, int64_t* allele_bytes,
                                      int64_t* n_child_vertices, int64_t* n_parent_vertices, int* kmer_words);
ldbg_status ldbg_variant_result_get(const ldbg_variant_result* r, const ldbg_variant_arrays* into);
/* the same into device memory, queued on `stream` (NULL: the default stream) without waiting for it */
ldbg_status ldbg_variant_result_get_dev(const ldbg_variant_result* r, const ldbg_variant_arrays* into, void* stream);
ldbg_status ldbg_variant_result_free(ldbg_variant_result* r);

/* ------------------------------------------------------------------ Tesserae: mosaic alignment in batches
 * J/utils/alignment/mosaic/Tesserae.java:95-382 — initialize, and alignAll up to the end of its traceback — for n independent problems in
 * one call (Call.java:119,177 aligns one section of one partition at a time).  Problem i aligns queries[query_off[i] .. query_off[i+1])
 * against the targets target_first[i] .. target_first[i+1] - 1 in that order (the panel's order after the query, :98-100); target t is
 * targets[target_off[t] .. target_off[t+1]).  target_first[0] must be 0.  Bytes other than T, C, A, G (lower case included) are the
 * fifth symbol (convert, :497-506).  The logs of :107-122 and :155,164,198 are taken once on the host; the device adds and compares
 * doubles in Java's order, so llk carries Java's bits wherever Math.log agrees with the C library's log.
 * Per problem: llk (:343) and maxpath_copy / maxpath_state / maxpath_pos[cp .. 2 maxl] after the loop of :354-380 (copy: 1-based index
 * into the panel, the query being 1; state: 1 match, 2 insert, 3 delete; pos: 1-based in that sequence), every step of it through the
 * encoding of :239,270-315 and the three casts of :363-365 in double.  The text tracks of :385-492 are built by the caller from these.
 * status[i] is LDBG_OK or LDBG_ERR_UNSUPPORTED; a refused problem has an empty path and llk 0 and leaves the others as they are:
 *   - an empty query, or no targets (the reference throws: :189, :198 of nothing), or targets without a single base (:440 throws);
 *   - maxl <= 2, maxl the longest of query and targets: tb_divisor is 1 and :239 packs positions into the state digit;
 *   - a problem whose traceback bytes (query length x sum of target lengths, plus 49 bytes per cell of a column when the columns do
 *     not fit LDS) exceed the arena budget: a quarter of the free device memory, or LDBG_MOSAIC_ARENA_BYTES;
 *   - a traceback that leaves the reference's arrays (ArrayIndexOutOfBoundsException at :356-371: more than 2 maxl steps, or a decoded
 *     position past maxl).
 * A batch runs in as many launches as the budget needs, one after another; its results do not depend on the split.
 * LDBG_ERR_ARG: n < 0, a null pointer, negative or decreasing offsets, target_first[0] != 0.  n == 0: an empty result. */
typedef struct { double del, eps, rho, term; } ldbg_mosaic_params;      /* Tesserae(del, eps, rho, term) (:87-92); the defaults of :14-17 are 0.025 0.75 1e-4 1e-3 */
typedef struct ldbg_mosaic_result ldbg_mosaic_result;
/* where ldbg_mosaic_result_get writes; any pointer may be NULL */
typedef struct {
    uint8_t* status;             /* [n] */
    double* llk;                 /* [n] getMaximumLogLikelihood (:508-510) */
    int64_t* path_off;           /* [n + 1] */
    int32_t* copy;               /* [path_entries] maxpath_copy */
    int32_t* state;              /* [path_entries] maxpath_state */
    int32_t* pos;                /* [path_entries] maxpath_pos */
} ldbg_mosaic_arrays;
ldbg_status ldbg_mosaic_align_batch(int device, const ldbg_mosaic_params* p, int64_t n, const char* queries, const int64_t* query_off,
                                    const int64_t* target_first, const char* targets, const int64_t* target_off, ldbg_mosaic_result** out);
ldbg_status ldbg_mosaic_result_sizes(const ldbg_mosaic_result* r, int64_t* n, int64_t* path_entries);
ldbg_status ldbg_mosaic_result_get(const ldbg_mosaic_result* r, const ldbg_mosaic_arrays* into);
ldbg_status ldbg_mosaic_result_free(ldbg_mosaic_result* r);
/* (who * 10 + state) + pos / div of :270 followed by the casts of :363-365, as the kernel computes them, for n triples: out[3n] = who,
 * state, pos as decoded (they differ from the input where the double runs out of digits) */
ldbg_status ldbg_mosaic_tb_roundtrip(int device, double div, int64_t n, const int32_t* who, const int32_t* state, const int32_t* pos, int32_t* out);

/* ------------------------------------------------------------------ Smith-Waterman: pairwise local alignment in batches
 * J/utils/alignment/sw/SmithWaterman.java:89-294 — align(Sequence, Sequence) with EDNAFULL: the three-state recurrences, getMaxScorePos
 * and the traceback — for n independent pairs in one call (Call.java:1171-1172, VerifyCalls.java:77-78 and EvaluateCalls2.java:205-219
 * align one pair at a time).  Pair i aligns queries[query_off[i] .. query_off[i+1]) against subjects[subject_off[i] .. subject_off[i+1]).
 * The bytes are what align(String, String) (:46-71) hands to Sequence.add after its header regex (the caller strips the header);
 * Sequence.add (Sequence.java:48-61: \r and \n dropped) and EDNAFULL.filter (EDNAFULL.java:63-80: NUL, '-' and '.' dropped, the 16
 * letters ATGCSWRYKMBVHDN* kept, any other byte 'X') are applied here.  A pair with an 'X' on either side scores 10000, the fill of
 * EDNAFULL.scoreMat (:35-39).  The device computes in int32 half units (every operand of the Java is a multiple of 0.5), so score
 * carries Java's bits.
 * Per pair: score (SWResult.score; -1 for the empty result of :190-192), the cell of the maximum end_q / end_s (:274-294, 1-based into
 * the filtered letters), begin_q / begin_s (lx / ly after the loop of :205-234), the columns the traceback appended in alignment order
 * (0: both letters, 1: '-' in the query, 2: '-' in the subject), aligned_len (the length of SWResult.qseq with the unaligned ends of
 * :237-259) and edits (the columns whose two characters differ, as Call.java:1174-1179 counts them).  The empty result has ends -1, no
 * column, aligned_len 0; an empty query or subject gives it too.
 * status[i] is LDBG_OK or LDBG_ERR_UNSUPPORTED; a refused pair has the empty result's values and leaves the others as they are:
 *   - min(|q|, |s|) >= 107,374 (10000 per column could pass 2^31 half units), or a side of 2^30 letters or more: before any budget;
 *   - a pair whose traceback bytes (one per cell, in strips of 64 rows of |s| + 63 steps, plus 12 bytes per subject letter when
 *     the boundary row does not fit LDS) exceed the arena budget: a quarter of the free device memory, or LDBG_SW_ARENA_BYTES.
 * A batch runs in as many launches as the budget needs, one after another; its results do not depend on the split.  A batch without
 * a pair for the device allocates nothing there.
 * LDBG_ERR_ARG: n < 0, a null pointer, negative or decreasing offsets.  n == 0: an empty result. */
typedef struct ldbg_sw_result ldbg_sw_result;
/* where ldbg_sw_result_get writes; any pointer may be NULL */
typedef struct {
    uint8_t* status;             /* [n] */
    double* score;               /* [n] SWResult.score */
    int32_t* end_q;              /* [n] */
    int32_t* end_s;              /* [n] */
    int32_t* begin_q;            /* [n] */
    int32_t* begin_s;            /* [n] */
    int32_t* aligned_len;        /* [n] */
    int32_t* edits;              /* [n] */
    int64_t* col_off;            /* [n + 1] */
    uint8_t* cols;               /* [columns] */
    int64_t* q_off;              /* [n + 1] */
    uint8_t* q_letters;          /* [query_letters] EDNAFULL.filter of the queries */
    int64_t* s_off;              /* [n + 1] */
    uint8_t* s_letters;          /* [subject_letters] */
} ldbg_sw_arrays;
ldbg_status ldbg_sw_align_batch(int device, int64_t n, const char* queries, const int64_t* query_off, const char* subjects,
                                const int64_t* subject_off, ldbg_sw_result** out);
ldbg_status ldbg_sw_result_sizes(const ldbg_sw_result* r, int64_t* n, int64_t* columns, int64_t* query_letters, int64_t* subject_letters);
ldbg_status ldbg_sw_result_get(const ldbg_sw_result* r, const ldbg_sw_arrays* into);
ldbg_status ldbg_sw_result_free(ldbg_sw_result* r);

/* ------------------------------------------------------------------ measurement hooks (bench.py)
 * average device time (ms, HIP events on the launch stream) and launch count of the named kernel
 * family since the last reset: "find", "records", "walk", "dfs", "contig", "unitigs", "select" (the selection kernels of one
 * ldbg_graph_select), "select_pack" (the gather of one ldbg_selection_write_ctx / _open_graph),
 * "recover" (the kernels of one ldbg_graph_recover other than its findRecord launch, which counts under "find"), "cursor" (the kernels
 * of one ldbg_engine_cursor_batch; "cursor_steps" and "cursor_longest" carry the steps of a batch and of its longest cursor as the
 * "ms" figure), "seeds" (the kernels of one ldbg_graph_variant_seeds), "occurrences" (the kernel of one ldbg_threading_occurrences), "variants" (the
 * kernels of one ldbg_engine_variant_batch other than its two cursor batches, which count under "cursor"), "mosaic" (the launches of one
 * ldbg_mosaic_align_batch), "sw" (the launches of one ldbg_sw_align_batch). */
ldbg_status ldbg_profile_reset(void);
ldbg_status ldbg_profile_get(const char* family, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* LDBG_H */
