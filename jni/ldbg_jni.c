/* JNI glue for a Java host: the classes under jni/java/uk/ac/ox/well/cortexjdk/gpu/ (GpuCortexGraph implements DeBruijnGraph,
 * GpuCortexLinks implements ConnectivityAnnotations, GpuTraversalEngine mirrors the TraversalEngine facade, GpuCortexTools = Sort /
 * Join / FindROIs / FindLowCoverage / FindDust / FindShared / Remove / contigs threaded through a graph) declare these natives, which call the C ABI of include/ldbg.h one to one.  This repository's image has no JDK, so the glue
 * is shipped as source; tests/test_jni_glue.py checks that it compiles against a declaration-only jni.h (tests/jni_stub), that
 * every `native` method of the Java classes has its Java_... definition here and that every ldbg_* entry point a Java host needs is
 * called.  Build on a host with a JDK:
 *   gcc -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -Iinclude jni/ldbg_jni.c -Lcorticall_amd/_build -lldbg -o libldbg_jni.so
 * Non-zero statuses are rethrown as the exception the reference would have thrown. */
#include <jni.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "ldbg.h"

#define G(h) ((ldbg_graph*)(intptr_t)(h))
#define L(h) ((ldbg_links*)(intptr_t)(h))
#define E(h) ((ldbg_engine*)(intptr_t)(h))
#define R(h) ((ldbg_dfs_result*)(intptr_t)(h))
#define JNIFN(cls, name) JNIEXPORT JNICALL Java_uk_ac_ox_well_cortexjdk_gpu_##cls##_##name

static void rethrow(JNIEnv* env, ldbg_status st) {
    const char* cls = "uk/ac/ox/well/cortexjdk/utils/exceptions/CortexJDKException";
    if (st == LDBG_ERR_NULLPOINTER) cls = "java/lang/NullPointerException";
    else if (st == LDBG_ERR_NOSUCHELEMENT) cls = "java/util/NoSuchElementException";
    else if (st == LDBG_ERR_UNSUPPORTED) cls = "java/lang/UnsupportedOperationException";
    else if (st == LDBG_ERR_ARG) cls = "java/lang/IllegalArgumentException";
    jclass c = (*env)->FindClass(env, cls);
    if (!c) { (*env)->ExceptionClear(env); c = (*env)->FindClass(env, "java/lang/RuntimeException"); }
    if (c) (*env)->ThrowNew(env, c, ldbg_last_error());
}
#define CHECK(call, ret) do { ldbg_status st__ = (call); if (st__ != LDBG_OK) { rethrow(env, st__); return ret; } } while (0)
static jstring cstr(JNIEnv* env, const char* s) { return (*env)->NewStringUTF(env, s); }

/* ------------------------------------------------------------------ GpuCortexGraph: DeBruijnGraph.java:16-53 */
jlong JNIFN(GpuCortexGraph, open)(JNIEnv* env, jclass c, jstring path, jint device) {
    const char* p = (*env)->GetStringUTFChars(env, path, NULL);
    ldbg_graph* g = NULL;
    ldbg_status st = ldbg_graph_open(p, device, &g);
    (*env)->ReleaseStringUTFChars(env, path, p);
    if (st != LDBG_OK) { rethrow(env, st); return 0; }
    return (jlong)(intptr_t)g;
}
/* new CortexCollection(graphs...): the members merged into one resident table; findView: the graph findRecord answers from */
jlong JNIFN(GpuCortexGraph, openCollection)(JNIEnv* env, jclass c, jobjectArray ins, jboolean findView, jint device) {
    jsize np = (*env)->GetArrayLength(env, ins);
    const char** paths = (const char**)calloc((size_t)(np > 0 ? np : 1), sizeof(*paths));
    jstring* held = (jstring*)calloc((size_t)(np > 0 ? np : 1), sizeof(*held));
    for (jsize i = 0; i < np; i++) { held[i] = (jstring)(*env)->GetObjectArrayElement(env, ins, i); paths[i] = (*env)->GetStringUTFChars(env, held[i], NULL); }
    ldbg_graph* g = NULL;
    ldbg_status st = ldbg_graph_open_collection(paths, (int)np, findView ? 1 : 0, device, &g);
    for (jsize i = 0; i < np; i++) (*env)->ReleaseStringUTFChars(env, held[i], paths[i]);
    free(paths); free(held);
    if (st != LDBG_OK) { rethrow(env, st); return 0; }
    return (jlong)(intptr_t)g;
}
void JNIFN(GpuCortexGraph, close)(JNIEnv* env, jclass c, jlong h) { CHECK(ldbg_graph_close(G(h)), ); }
/* getKmerSize / getKmerBits / getNumColors / getNumRecords / getVersion as a long[5] */
jlongArray JNIFN(GpuCortexGraph, info)(JNIEnv* env, jclass c, jlong h) {
    int k, W, C, v; int64_t N;
    CHECK(ldbg_graph_info(G(h), &k, &W, &C, &N, &v), NULL);
    jlong vals[5] = {k, W, C, N, v};
    jlongArray out = (*env)->NewLongArray(env, 5);
    if (out) (*env)->SetLongArrayRegion(env, out, 0, 5, vals);
    return out;
}
jstring JNIFN(GpuCortexGraph, sampleName)(JNIEnv* env, jclass c, jlong h, jint color) {
    char buf[4096];
    CHECK(ldbg_graph_sample_name(G(h), color, buf, (int)sizeof buf), NULL);
    return cstr(env, buf);
}
/* CortexColor fields of one colour: {meanReadLength, totalSequence, tipClipping, lowCovgSupernodesRemoved, lowCovgKmersRemoved,
 * cleanedAgainstGraph, lowCovSupernodesThreshold, lowCovKmerThreshold}; the cleaned-against graph name through nameOut[0] */
jlongArray JNIFN(GpuCortexGraph, colorInfo)(JNIEnv* env, jclass c, jlong h, jint color, jobjectArray nameOut) {
    ldbg_color_info ci;
    char name[4096];
    CHECK(ldbg_graph_color_info(G(h), color, &ci, name, (int)sizeof name), NULL);
    jlong vals[8] = {ci.mean_read_length, (jlong)ci.total_sequence, ci.tip_clipping, ci.low_covg_supernodes_removed, ci.low_covg_kmers_removed,
                     ci.cleaned_against_graph, ci.low_cov_supernodes_threshold, ci.low_cov_kmer_threshold};
    jlongArray out = (*env)->NewLongArray(env, 8);
    if (out) (*env)->SetLongArrayRegion(env, out, 0, 8, vals);
    if (nameOut) (*env)->SetObjectArrayElement(env, nameOut, 0, cstr(env, name));
    return out;
}
jint JNIFN(GpuCortexGraph, colorForSampleName)(JNIEnv* env, jclass c, jlong h, jstring name) {
    const char* p = (*env)->GetStringUTFChars(env, name, NULL);
    int color = -1;
    ldbg_status st = ldbg_graph_color_for_sample_name(G(h), p, &color);
    (*env)->ReleaseStringUTFChars(env, name, p);
    if (st != LDBG_OK) { rethrow(env, st); return -1; }
    return color;
}
/* findRecord in bulk: kmers = n*k ASCII bytes; returns record indices (-1 = null), fills cov (n*C ints) and edges (n*C bytes) */
jlongArray JNIFN(GpuCortexGraph, findRecords)(JNIEnv* env, jclass c, jlong h, jbyteArray kmers, jint n, jintArray cov, jbyteArray edges) {
    jbyte* km = (*env)->GetByteArrayElements(env, kmers, NULL);
    jint* cv = (*env)->GetIntArrayElements(env, cov, NULL);
    jbyte* ed = (*env)->GetByteArrayElements(env, edges, NULL);
    int64_t* idx = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1));
    ldbg_status st = ldbg_graph_find_ascii(G(h), (const char*)km, n, idx, (uint32_t*)cv, (uint8_t*)ed);
    (*env)->ReleaseByteArrayElements(env, kmers, km, JNI_ABORT);
    (*env)->ReleaseIntArrayElements(env, cov, cv, 0);
    (*env)->ReleaseByteArrayElements(env, edges, ed, 0);
    jlongArray out = NULL;
    if (st == LDBG_OK) { out = (*env)->NewLongArray(env, n); if (out) (*env)->SetLongArrayRegion(env, out, 0, n, (const jlong*)idx); }
    free(idx);
    if (st != LDBG_OK) rethrow(env, st);
    return out;
}
/* Iterator<CortexRecord> / getRecord in bulk */
void JNIFN(GpuCortexGraph, records)(JNIEnv* env, jclass c, jlong h, jlong first, jint n, jlongArray words, jintArray cov, jbyteArray edges) {
    jlong* w = (*env)->GetLongArrayElements(env, words, NULL);
    jint* cv = (*env)->GetIntArrayElements(env, cov, NULL);
    jbyte* ed = (*env)->GetByteArrayElements(env, edges, NULL);
    ldbg_status st = ldbg_graph_records(G(h), first, n, (uint64_t*)w, (uint32_t*)cv, (uint8_t*)ed);
    (*env)->ReleaseLongArrayElements(env, words, w, 0);
    (*env)->ReleaseIntArrayElements(env, cov, cv, 0);
    (*env)->ReleaseByteArrayElements(env, edges, ed, 0);
    if (st != LDBG_OK) rethrow(env, st);
}

/* ------------------------------------------------------------------ GpuCortexLinks: ConnectivityAnnotations.java:15-45 */
jlong JNIFN(GpuCortexLinks, open)(JNIEnv* env, jclass c, jstring path, jlong graph) {
    const char* p = (*env)->GetStringUTFChars(env, path, NULL);
    ldbg_links* l = NULL;
    ldbg_status st = ldbg_links_open(p, G(graph), &l);
    (*env)->ReleaseStringUTFChars(env, path, p);
    if (st != LDBG_OK) { rethrow(env, st); return 0; }
    return (jlong)(intptr_t)l;
}
void JNIFN(GpuCortexLinks, close)(JNIEnv* env, jclass c, jlong h) { CHECK(ldbg_links_close(L(h)), ); }
/* {version, numColors, kmerSize, numKmersInGraph, numKmersWithLinks, numLinks} */
jlongArray JNIFN(GpuCortexLinks, info)(JNIEnv* env, jclass c, jlong h) {
    int v, nc, k; int64_t a, b, d;
    CHECK(ldbg_links_info(L(h), &v, &nc, &k, &a, &b, &d), NULL);
    jlong vals[6] = {v, nc, k, a, b, d};
    jlongArray out = (*env)->NewLongArray(env, 6);
    if (out) (*env)->SetLongArrayRegion(env, out, 0, 6, vals);
    return out;
}
jstring JNIFN(GpuCortexLinks, sampleName)(JNIEnv* env, jclass c, jlong h, jint color) {
    char buf[4096];
    CHECK(ldbg_links_sample_name(L(h), color, buf, (int)sizeof buf), NULL);
    return cstr(env, buf);
}
/* get(key): the record as the text lines of the link file ("KMER n" + one line per junction record, in the reference's HashSet order),
 * or null when the k-mer has no links (containsKey == false) */
jstring JNIFN(GpuCortexLinks, get)(JNIEnv* env, jclass c, jlong h, jbyteArray kmer) {
    jsize k = (*env)->GetArrayLength(env, kmer);
    char* km = (char*)malloc((size_t)k + 1);
    (*env)->GetByteArrayRegion(env, kmer, 0, k, (jbyte*)km);
    km[k] = 0;
    int found = 0;
    int64_t cap = 1 << 16;
    char* buf = (char*)malloc((size_t)cap);
    ldbg_status st = ldbg_links_get(L(h), km, &found, buf, cap);
    while (st == LDBG_ERR_CAPACITY && cap < (1LL << 30)) { cap *= 8; buf = (char*)realloc(buf, (size_t)cap); st = ldbg_links_get(L(h), km, &found, buf, cap); }
    jstring out = NULL;
    if (st == LDBG_OK && found) out = cstr(env, buf);
    free(buf); free(km);
    if (st != LDBG_OK) rethrow(env, st);
    return out;
}

/* ------------------------------------------------------------------ GpuTraversalEngine: TraversalEngine.java:33-339 */
/* TraversalEngineFactory.make(): colours as int[]; links as long[] of handles (the engine itself refuses more than it supports) */
jlong JNIFN(GpuTraversalEngine, create)(JNIEnv* env, jclass c, jlong graph, jlong rois, jlongArray links, jintArray trav, jintArray join,
        jintArray recruit, jintArray secondary, jint direction, jint op, jint stopper, jint maxLen, jboolean connectAll) {
    ldbg_engine_config cfg;
    ldbg_engine_config_default(&cfg);
    cfg.graph = G(graph);
    cfg.rois = G(rois);
    jsize nl = links ? (*env)->GetArrayLength(env, links) : 0;
    const ldbg_links** lk = (const ldbg_links**)calloc((size_t)(nl > 0 ? nl : 1), sizeof(*lk));
    if (nl) { jlong* p = (*env)->GetLongArrayElements(env, links, NULL); for (jsize i = 0; i < nl; i++) lk[i] = L(p[i]); (*env)->ReleaseLongArrayElements(env, links, p, JNI_ABORT); }
    cfg.links = lk; cfg.nlinks = (int)nl;
#define COPY_COLOURS(arr, dst, cnt) do { jsize n_ = (arr) ? (*env)->GetArrayLength(env, (arr)) : 0; \
        if (n_ > LDBG_MAX_COLORS) { free(lk); rethrow(env, LDBG_ERR_ARG); return 0; } \
        if (n_) { (*env)->GetIntArrayRegion(env, (arr), 0, n_, (jint*)(dst)); } \
        (cnt) = (int)n_; } while (0)
    COPY_COLOURS(trav, cfg.traversal_colors, cfg.n_traversal);
    COPY_COLOURS(join, cfg.joining_colors, cfg.n_joining);
    COPY_COLOURS(recruit, cfg.recruitment_colors, cfg.n_recruitment);
    COPY_COLOURS(secondary, cfg.secondary_colors, cfg.n_secondary);
    cfg.direction = direction; cfg.combination_operator = op; cfg.stopping_rule = stopper;
    cfg.max_branch_length = maxLen; cfg.connect_all_neighbors = connectAll ? 1 : 0;
    ldbg_engine* e = NULL;
    ldbg_status st = ldbg_engine_create(&cfg, &e);
    free(lk);
    if (st != LDBG_OK) { rethrow(env, st); return 0; }
    return (jlong)(intptr_t)e;
}
void JNIFN(GpuTraversalEngine, destroy)(JNIEnv* env, jclass c, jlong h) { CHECK(ldbg_engine_destroy(E(h)), ); }
/* walk(seed) + toContig for n seeds: returns the contigs back to back; offsets[n+1]; walkLen[n] vertices per walk */
jbyteArray JNIFN(GpuTraversalEngine, walkBatch)(JNIEnv* env, jclass c, jlong h, jbyteArray seeds, jint n, jlongArray offsets, jlongArray walkLen) {
    jbyte* sd = (*env)->GetByteArrayElements(env, seeds, NULL);
    int64_t total = 0, trav = 0;
    ldbg_status st = ldbg_engine_walk_batch_run(E(h), (const char*)sd, n, &total, &trav);
    (*env)->ReleaseByteArrayElements(env, seeds, sd, JNI_ABORT);
    if (st != LDBG_OK) { rethrow(env, st); return NULL; }
    jbyteArray out = (*env)->NewByteArray(env, (jsize)total);
    if (!out) return NULL;
    jbyte* o = (*env)->GetByteArrayElements(env, out, NULL);
    jlong* off = (*env)->GetLongArrayElements(env, offsets, NULL);
    jlong* wl = walkLen ? (*env)->GetLongArrayElements(env, walkLen, NULL) : NULL;
    st = ldbg_engine_walk_batch_fetch(E(h), (char*)o, total, (int64_t*)off, (int64_t*)wl);
    (*env)->ReleaseByteArrayElements(env, out, o, 0);
    (*env)->ReleaseLongArrayElements(env, offsets, off, 0);
    if (wl) (*env)->ReleaseLongArrayElements(env, walkLen, wl, 0);
    if (st != LDBG_OK) { rethrow(env, st); return NULL; }
    return out;
}
/* List<CortexVertex> of walk i of the last batch: returns the number of vertices; with arrays of that capacity fills k-mer words
 * (len x W), record index (-1 = null CortexRecord), copyIndex, index.  Call with capacity 0 (arrays null) to learn the length. */
jlong JNIFN(GpuTraversalEngine, walkVertices)(JNIEnv* env, jclass c, jlong h, jlong walk, jlong capacity, jlongArray words, jlongArray rec,
        jintArray copyIndex, jintArray index) {
    int64_t len = 0;
    if (capacity <= 0 || !words) {
        ldbg_status st = ldbg_engine_walk_vertices(E(h), walk, 0, &len, NULL, NULL, NULL, NULL);
        if (st != LDBG_OK && st != LDBG_ERR_CAPACITY) { rethrow(env, st); return -1; }
        return len;
    }
    jlong* w = (*env)->GetLongArrayElements(env, words, NULL);
    jlong* r = (*env)->GetLongArrayElements(env, rec, NULL);
    jint* ci = (*env)->GetIntArrayElements(env, copyIndex, NULL);
    jint* ix = (*env)->GetIntArrayElements(env, index, NULL);
    ldbg_status st = ldbg_engine_walk_vertices(E(h), walk, capacity, &len, (uint64_t*)w, (int64_t*)r, (int32_t*)ci, (int32_t*)ix);
    (*env)->ReleaseLongArrayElements(env, words, w, 0);
    (*env)->ReleaseLongArrayElements(env, rec, r, 0);
    (*env)->ReleaseIntArrayElements(env, copyIndex, ci, 0);
    (*env)->ReleaseIntArrayElements(env, index, ix, 0);
    if (st != LDBG_OK) { rethrow(env, st); return -1; }
    return len;
}
/* Partition.markUsedRois inputs: ROI record numbers every walk of the last batch passes through; offsets[n+1]; hasNull[n] */
jintArray JNIFN(GpuTraversalEngine, walkRoiHits)(JNIEnv* env, jclass c, jlong h, jint n, jlongArray offsets, jbyteArray hasNull) {
    jlong* off = (*env)->GetLongArrayElements(env, offsets, NULL);
    jbyte* hn = (*env)->GetByteArrayElements(env, hasNull, NULL);
    int64_t cap = 1 << 16;
    uint32_t* hits = (uint32_t*)malloc((size_t)cap * 4);
    ldbg_status st = ldbg_engine_walk_roi_hits(E(h), (int64_t*)off, hits, cap, (uint8_t*)hn);
    if (st == LDBG_ERR_CAPACITY) { cap = off[n]; hits = (uint32_t*)realloc(hits, (size_t)(cap > 0 ? cap : 1) * 4); st = ldbg_engine_walk_roi_hits(E(h), (int64_t*)off, hits, cap, (uint8_t*)hn); }
    jintArray out = NULL;
    if (st == LDBG_OK) { out = (*env)->NewIntArray(env, (jsize)off[n]); if (out) (*env)->SetIntArrayRegion(env, out, 0, (jsize)off[n], (const jint*)hits); }
    free(hits);
    (*env)->ReleaseLongArrayElements(env, offsets, off, 0);
    (*env)->ReleaseByteArrayElements(env, hasNull, hn, 0);
    if (st != LDBG_OK) rethrow(env, st);
    return out;
}
/* seek / hasNext / hasPrevious / next / previous: TraversalEngine.java:241-339 */
void JNIFN(GpuTraversalEngine, seek)(JNIEnv* env, jclass c, jlong h, jbyteArray kmer) {
    jsize k = (*env)->GetArrayLength(env, kmer);
    char* km = (char*)malloc((size_t)k + 1);
    (*env)->GetByteArrayRegion(env, kmer, 0, k, (jbyte*)km);
    km[k] = 0;
    ldbg_status st = ldbg_engine_seek(E(h), km);
    free(km);
    if (st != LDBG_OK) rethrow(env, st);
}
jboolean JNIFN(GpuTraversalEngine, hasNext)(JNIEnv* env, jclass c, jlong h) {
    int yes = 0;
    CHECK(ldbg_engine_has_next(E(h), &yes), JNI_FALSE);
    return yes ? JNI_TRUE : JNI_FALSE;
}
jboolean JNIFN(GpuTraversalEngine, hasPrevious)(JNIEnv* env, jclass c, jlong h) {
    int yes = 0;
    CHECK(ldbg_engine_has_previous(E(h), &yes), JNI_FALSE);
    return yes ? JNI_TRUE : JNI_FALSE;
}
static jlong cursor_step(JNIEnv* env, jlong h, jbyteArray kmerOut, int forward) {
    jsize k = (*env)->GetArrayLength(env, kmerOut);
    char* km = (char*)malloc((size_t)k + 1);
    int64_t rec = -1;
    ldbg_status st = forward ? ldbg_engine_next(E(h), km, &rec) : ldbg_engine_previous(E(h), km, &rec);
    if (st == LDBG_OK) (*env)->SetByteArrayRegion(env, kmerOut, 0, k, (const jbyte*)km);
    free(km);
    if (st != LDBG_OK) { rethrow(env, st); return -1; }
    return rec;
}
jlong JNIFN(GpuTraversalEngine, next)(JNIEnv* env, jclass c, jlong h, jbyteArray kmerOut) { return cursor_step(env, h, kmerOut, 1); }
jlong JNIFN(GpuTraversalEngine, previous)(JNIEnv* env, jclass c, jlong h, jbyteArray kmerOut) { return cursor_step(env, h, kmerOut, 0); }
/* dfs(source, sinks...) for n sources: sinks as CSR over ASCII k-mers (sinkOffsets[n+1], may be null) -> result handle */
jlong JNIFN(GpuTraversalEngine, dfsBatch)(JNIEnv* env, jclass c, jlong h, jbyteArray sources, jint n, jbyteArray sinks, jlongArray sinkOffsets) {
    jbyte* src = (*env)->GetByteArrayElements(env, sources, NULL);
    jbyte* sk = sinks ? (*env)->GetByteArrayElements(env, sinks, NULL) : NULL;
    jlong* so = sinkOffsets ? (*env)->GetLongArrayElements(env, sinkOffsets, NULL) : NULL;
    ldbg_dfs_result* r = NULL;
    ldbg_status st = ldbg_engine_dfs_batch(E(h), (const char*)src, n, (const char*)sk, (const int64_t*)so, &r);
    (*env)->ReleaseByteArrayElements(env, sources, src, JNI_ABORT);
    if (sk) (*env)->ReleaseByteArrayElements(env, sinks, sk, JNI_ABORT);
    if (so) (*env)->ReleaseLongArrayElements(env, sinkOffsets, so, JNI_ABORT);
    if (st != LDBG_OK) { rethrow(env, st); return 0; }
    return (jlong)(intptr_t)r;
}
/* dfs(Collection<String> sources, Collection<String> sinks) (TraversalEngine.java:37-62): results 0 .. n-1 of `res` merged in that order
 * with Graphs.addGraph -> a result handle holding ONE graph (index 0) */
jlong JNIFN(GpuTraversalEngine, dfsMerge)(JNIEnv* env, jclass c, jlong res, jint n) {
    int64_t* which = (int64_t*)malloc((size_t)(n > 0 ? n : 1) * 8);
    for (jint i = 0; i < n; i++) which[i] = i;
    ldbg_dfs_result* out = NULL;
    ldbg_status st = ldbg_dfs_result_merge(R(res), which, n, &out);
    free(which);
    if (st != LDBG_OK) { rethrow(env, st); return 0; }
    return (jlong)(intptr_t)out;
}
/* getNextVertices / getPrevVertices (TraversalEngine.java:147-239) of n k-mers: offsets[n+1]; words[4 n W], rec[4 n] filled up to offsets[n] */
void JNIFN(GpuTraversalEngine, neighboursBatch)(JNIEnv* env, jclass c, jlong h, jbyteArray kmers, jint n, jboolean forward, jlongArray offsets, jlongArray words, jlongArray rec) {
    jbyte* km = (*env)->GetByteArrayElements(env, kmers, NULL);
    jlong* off = (*env)->GetLongArrayElements(env, offsets, NULL);
    jlong* w = (*env)->GetLongArrayElements(env, words, NULL);
    jlong* r = (*env)->GetLongArrayElements(env, rec, NULL);
    ldbg_status st = ldbg_engine_neighbours_batch(E(h), (const char*)km, n, forward ? 1 : 0, (int64_t*)off, (uint64_t*)w, (int64_t*)r, 4 * (int64_t)n);
    (*env)->ReleaseByteArrayElements(env, kmers, km, JNI_ABORT);
    (*env)->ReleaseLongArrayElements(env, offsets, off, 0);
    (*env)->ReleaseLongArrayElements(env, words, w, 0);
    (*env)->ReleaseLongArrayElements(env, rec, r, 0);
    if (st != LDBG_OK) rethrow(env, st);
}
/* assemble(seed) (TraversalEngine.java:112-145): returns the number of vertices; with arrays of that capacity fills words (len x W) and rec */
jlong JNIFN(GpuTraversalEngine, assemble)(JNIEnv* env, jclass c, jlong h, jbyteArray seed, jlong capacity, jlongArray words, jlongArray rec) {
    jsize k = (*env)->GetArrayLength(env, seed);
    char* sd = (char*)malloc((size_t)k + 1);
    (*env)->GetByteArrayRegion(env, seed, 0, k, (jbyte*)sd);
    sd[k] = 0;
    int64_t len = 0;
    ldbg_status st;
    if (capacity <= 0 || !words) {
        st = ldbg_engine_assemble(E(h), sd, 0, &len, NULL, NULL);
        free(sd);
        if (st != LDBG_OK && st != LDBG_ERR_CAPACITY) { rethrow(env, st); return -1; }
        return len;
    }
    jlong* w = (*env)->GetLongArrayElements(env, words, NULL);
    jlong* r = (*env)->GetLongArrayElements(env, rec, NULL);
    st = ldbg_engine_assemble(E(h), sd, capacity, &len, (uint64_t*)w, (int64_t*)r);
    free(sd);
    (*env)->ReleaseLongArrayElements(env, words, w, 0);
    (*env)->ReleaseLongArrayElements(env, rec, r, 0);
    if (st != LDBG_OK) { rethrow(env, st); return -1; }
    return len;
}
/* assembleBatch: n cursors advanced to their end in one call (ldbg_engine_cursor_batch; TraversalEngine.java:112-145 per seed) -> a result
 * handle.  colour < 0: no colour rule; targets may be null */
#define CR(h) ((ldbg_cursor_result*)(intptr_t)(h))
jlong JNIFN(GpuTraversalEngine, cursorBatch)(JNIEnv* env, jclass c, jlong h, jbyteArray seeds, jint n, jint direction, jlong maxSteps, jint colour,
                                            jboolean arrivalDegreeOne, jbyteArray targets) {
    if (!seeds) { rethrow(env, LDBG_ERR_NULLPOINTER); return 0; }
    jbyte* sd = (*env)->GetByteArrayElements(env, seeds, NULL);
    jbyte* tg = targets ? (*env)->GetByteArrayElements(env, targets, NULL) : NULL;
    ldbg_cursor_stop stop;
    stop.colour = colour; stop.arrival_degree_one = arrivalDegreeOne ? 1 : 0; stop.targets = (const char*)tg;
    ldbg_cursor_result* r = NULL;
    ldbg_status st = ldbg_engine_cursor_batch(E(h), (const char*)sd, n, direction, maxSteps, &stop, &r);
    (*env)->ReleaseByteArrayElements(env, seeds, sd, JNI_ABORT);
    if (tg) (*env)->ReleaseByteArrayElements(env, targets, tg, JNI_ABORT);
    if (st != LDBG_OK) { rethrow(env, st); return 0; }
    return (jlong)(intptr_t)r;
}
/* {seeds, vertices, words per k-mer} of a cursor result */
jlongArray JNIFN(GpuTraversalEngine, cursorSizes)(JNIEnv* env, jclass c, jlong res) {
    int64_t ns = 0, nv = 0; int w = 0;
    CHECK(ldbg_cursor_result_sizes(CR(res), &ns, &nv, &w), NULL);
    jlong vals[3] = {ns, nv, w};
    jlongArray out = (*env)->NewLongArray(env, 3);
    if (out) (*env)->SetLongArrayRegion(env, out, 0, 3, vals);
    return out;
}
/* offsets[n + 1], words[vertices x W], rec[vertices], nReverse[n], nForward[n], seedRec[n], ends[2 n] (reverse, then forward), status[n] */
void JNIFN(GpuTraversalEngine, cursorGet)(JNIEnv* env, jclass c, jlong res, jlongArray offsets, jlongArray words, jlongArray rec, jintArray nReverse,
                                         jintArray nForward, jlongArray seedRec, jbyteArray ends, jbyteArray status) {
    if (!offsets || !words || !rec || !nReverse || !nForward || !seedRec || !ends || !status) { rethrow(env, LDBG_ERR_NULLPOINTER); return; }
    int64_t ns = 0;
    CHECK(ldbg_cursor_result_sizes(CR(res), &ns, NULL, NULL), );
    jlong* off = (*env)->GetLongArrayElements(env, offsets, NULL);
    jlong* w = (*env)->GetLongArrayElements(env, words, NULL);
    jlong* r = (*env)->GetLongArrayElements(env, rec, NULL);
    jint* nr = (*env)->GetIntArrayElements(env, nReverse, NULL);
    jint* nf = (*env)->GetIntArrayElements(env, nForward, NULL);
    jlong* sr = (*env)->GetLongArrayElements(env, seedRec, NULL);
    jbyte* en = (*env)->GetByteArrayElements(env, ends, NULL);
    jbyte* stt = (*env)->GetByteArrayElements(env, status, NULL);
    ldbg_status st = ldbg_cursor_result_get(CR(res), (int64_t*)off, (uint64_t*)w, (int64_t*)r, (int32_t*)nr, (int32_t*)nf, (int64_t*)sr, (uint8_t*)en,
                                            (uint8_t*)en + ns, (uint8_t*)stt);
    (*env)->ReleaseLongArrayElements(env, offsets, off, 0);
    (*env)->ReleaseLongArrayElements(env, words, w, 0);
    (*env)->ReleaseLongArrayElements(env, rec, r, 0);
    (*env)->ReleaseIntArrayElements(env, nReverse, nr, 0);
    (*env)->ReleaseIntArrayElements(env, nForward, nf, 0);
    (*env)->ReleaseLongArrayElements(env, seedRec, sr, 0);
    (*env)->ReleaseByteArrayElements(env, ends, en, 0);
    (*env)->ReleaseByteArrayElements(env, status, stt, 0);
    if (st != LDBG_OK) rethrow(env, st);
}
void JNIFN(GpuTraversalEngine, cursorFree)(JNIEnv* env, jclass c, jlong res) { CHECK(ldbg_cursor_result_free(CR(res)), ); }
/* {isNull, vertices, edges} of result i */
jlongArray JNIFN(GpuTraversalEngine, dfsSizes)(JNIEnv* env, jclass c, jlong res, jlong i) {
    int is_null = 1; int64_t nv = 0, ne = 0;
    CHECK(ldbg_dfs_result_sizes(R(res), i, &is_null, &nv, &ne), NULL);
    jlong vals[3] = {is_null, nv, ne};
    jlongArray out = (*env)->NewLongArray(env, 3);
    if (out) (*env)->SetLongArrayRegion(env, out, 0, 3, vals);
    return out;
}
/* the DirectedWeightedPseudograph of result i: vertices (k-mer words nv x W, record, copyIndex, index) and edges (source, target, colour) in insertion order */
void JNIFN(GpuTraversalEngine, dfsGet)(JNIEnv* env, jclass c, jlong res, jlong i, jlongArray words, jlongArray rec, jintArray copyIndex, jintArray index,
        jintArray edgeSrc, jintArray edgeDst, jintArray edgeColor) {
    jlong* w = (*env)->GetLongArrayElements(env, words, NULL);
    jlong* r = (*env)->GetLongArrayElements(env, rec, NULL);
    jint* ci = (*env)->GetIntArrayElements(env, copyIndex, NULL);
    jint* ix = (*env)->GetIntArrayElements(env, index, NULL);
    jint* es = (*env)->GetIntArrayElements(env, edgeSrc, NULL);
    jint* ed = (*env)->GetIntArrayElements(env, edgeDst, NULL);
    jint* ec = (*env)->GetIntArrayElements(env, edgeColor, NULL);
    ldbg_status st = ldbg_dfs_result_get(R(res), i, (uint64_t*)w, (int64_t*)r, (int32_t*)ci, (int32_t*)ix, (int32_t*)es, (int32_t*)ed, (int32_t*)ec);
    (*env)->ReleaseLongArrayElements(env, words, w, 0);
    (*env)->ReleaseLongArrayElements(env, rec, r, 0);
    (*env)->ReleaseIntArrayElements(env, copyIndex, ci, 0);
    (*env)->ReleaseIntArrayElements(env, index, ix, 0);
    (*env)->ReleaseIntArrayElements(env, edgeSrc, es, 0);
    (*env)->ReleaseIntArrayElements(env, edgeDst, ed, 0);
    (*env)->ReleaseIntArrayElements(env, edgeColor, ec, 0);
    if (st != LDBG_OK) rethrow(env, st);
}
/* TraversalUtils.toWalk(g, seed, colour) + toContig on result i */
jstring JNIFN(GpuTraversalEngine, dfsWalk)(JNIEnv* env, jclass c, jlong res, jlong i, jbyteArray seed, jint color) {
    jsize k = (*env)->GetArrayLength(env, seed);
    char* km = (char*)malloc((size_t)k + 1);
    (*env)->GetByteArrayRegion(env, seed, 0, k, (jbyte*)km);
    km[k] = 0;
    int64_t cap = 1 << 16, len = 0;
    char* buf = (char*)malloc((size_t)cap);
    ldbg_status st = ldbg_dfs_result_walk(R(res), i, km, color, buf, cap, &len);
    if (st == LDBG_ERR_CAPACITY) { cap = len + 16; buf = (char*)realloc(buf, (size_t)cap); st = ldbg_dfs_result_walk(R(res), i, km, color, buf, cap, &len); }
    jstring out = NULL;
    if (st == LDBG_OK) { buf[len < cap ? len : cap - 1] = 0; out = cstr(env, buf); }
    free(buf); free(km);
    if (st != LDBG_OK) rethrow(env, st);
    return out;
}
void JNIFN(GpuTraversalEngine, dfsFree)(JNIEnv* env, jclass c, jlong res) { CHECK(ldbg_dfs_result_free(R(res)), ); }
jlong JNIFN(GpuTraversalEngine, dfsKmersTraversed)(JNIEnv* env, jclass c, jlong h) {
    int64_t n = 0;
    CHECK(ldbg_engine_dfs_kmers_traversed(E(h), &n), 0);
    return n;
}

/* ------------------------------------------------------------------ GpuCortexTools: commands/utils/Sort.java:20-49, Join.java:16-60 */
jlong JNIFN(GpuCortexTools, sort)(JNIEnv* env, jclass c, jstring in, jstring out, jint device) {
    const char* a = (*env)->GetStringUTFChars(env, in, NULL);
    const char* b = (*env)->GetStringUTFChars(env, out, NULL);
    int64_t n = 0;
    ldbg_status st = ldbg_sort_ctx(a, b, device, &n);
    (*env)->ReleaseStringUTFChars(env, in, a);
    (*env)->ReleaseStringUTFChars(env, out, b);
    if (st != LDBG_OK) { rethrow(env, st); return -1; }
    return n;
}
jlong JNIFN(GpuCortexTools, join)(JNIEnv* env, jclass c, jobjectArray ins, jstring out, jint device) {
    jsize np = (*env)->GetArrayLength(env, ins);
    const char** paths = (const char**)calloc((size_t)(np > 0 ? np : 1), sizeof(*paths));
    jstring* held = (jstring*)calloc((size_t)(np > 0 ? np : 1), sizeof(*held));
    for (jsize i = 0; i < np; i++) { held[i] = (jstring)(*env)->GetObjectArrayElement(env, ins, i); paths[i] = (*env)->GetStringUTFChars(env, held[i], NULL); }
    const char* b = (*env)->GetStringUTFChars(env, out, NULL);
    int64_t n = 0;
    ldbg_status st = ldbg_join_ctx(paths, (int)np, b, device, &n);
    for (jsize i = 0; i < np; i++) (*env)->ReleaseStringUTFChars(env, held[i], paths[i]);
    (*env)->ReleaseStringUTFChars(env, out, b);
    free(paths); free(held);
    if (st != LDBG_OK) { rethrow(env, st); return -1; }
    return n;
}
/* CortexGraphWriter over a selection of records (FindTips.java:112-131 and the other filters) */
void JNIFN(GpuCortexTools, writeRecords)(JNIEnv* env, jclass c, jstring in, jlongArray indices, jstring out) {
    const char* a = (*env)->GetStringUTFChars(env, in, NULL);
    const char* b = (*env)->GetStringUTFChars(env, out, NULL);
    jsize n = (*env)->GetArrayLength(env, indices);
    jlong* idx = (*env)->GetLongArrayElements(env, indices, NULL);
    ldbg_status st = ldbg_ctx_write_records(a, (const int64_t*)idx, (int64_t)n, b);
    (*env)->ReleaseLongArrayElements(env, indices, idx, JNI_ABORT);
    (*env)->ReleaseStringUTFChars(env, in, a);
    (*env)->ReleaseStringUTFChars(env, out, b);
    if (st != LDBG_OK) { rethrow(env, st); }
}
/* TempLinksAssembler.buildLinks (J/utils/assembler/TempLinksAssembler.java:29): the reads back to back and their n + 1 offsets -> the link file; returns
 * {k-mers with links, links} */
jlongArray JNIFN(GpuCortexTools, buildLinks)(JNIEnv* env, jclass c, jlong graph, jstring sample, jbyteArray bases, jlongArray offsets, jstring out) {
    const char* s = (*env)->GetStringUTFChars(env, sample, NULL);
    const char* o = (*env)->GetStringUTFChars(env, out, NULL);
    jsize n = (*env)->GetArrayLength(env, offsets);
    jbyte* b = (*env)->GetByteArrayElements(env, bases, NULL);
    jlong* off = (*env)->GetLongArrayElements(env, offsets, NULL);
    int64_t r[2] = {0, 0};
    ldbg_status st = ldbg_links_build_ctp(G(graph), s, (const char*)b, (const int64_t*)off, n > 0 ? (int64_t)n - 1 : 0, 0, o, &r[0], &r[1]);
    (*env)->ReleaseLongArrayElements(env, offsets, off, JNI_ABORT);
    (*env)->ReleaseByteArrayElements(env, bases, b, JNI_ABORT);
    (*env)->ReleaseStringUTFChars(env, sample, s);
    (*env)->ReleaseStringUTFChars(env, out, o);
    if (st != LDBG_OK) { rethrow(env, st); return NULL; }
    jlongArray res = (*env)->NewLongArray(env, 2);
    jlong v[2] = {(jlong)r[0], (jlong)r[1]};
    (*env)->SetLongArrayRegion(env, res, 0, 2, v);
    return res;
}
jint JNIFN(GpuCortexTools, deviceCount)(JNIEnv* env, jclass c) {
    int n = 0;
    CHECK(ldbg_device_count(&n), 0);
    return n;
}

/* ------------------------------------------------------------------ GpuCortexTools: record selection (ldbg_graph_select)
 * FindROIs.java:30-82, FindLowCoverage.java:32-67, FindDust.java:78-135, FindShared.java:41-118, Remove.java:29-86: the records of
 * `graph` (or, query != 0, of `query` through graph.findRecord) that pass the filter — masks = {all_zero, all_positive, any_positive,
 * none_positive}, scalars = {cov_color, cov_below, degree_color, degree_above} — written to `out` reduced to `colours` under the
 * header of headerPath (null: the fresh header of FindROIs.makeCortexHeader).  Returns {records written, records tested}. */
static ldbg_record_filter filter_of(JNIEnv* env, jlongArray masks, jintArray scalars) {
    jlong* m = (*env)->GetLongArrayElements(env, masks, NULL);
    jint v[4];
    (*env)->GetIntArrayRegion(env, scalars, 0, 4, v);
    ldbg_record_filter f = {(uint64_t)m[0], (uint64_t)m[1], (uint64_t)m[2], (uint64_t)m[3], v[0], v[1], v[2], v[3]};
    (*env)->ReleaseLongArrayElements(env, masks, m, JNI_ABORT);
    return f;
}
jlongArray JNIFN(GpuCortexTools, selectWrite)(JNIEnv* env, jclass c, jlong graph, jlong query, jlongArray masks, jintArray scalars, jintArray colours,
                                              jstring headerPath, jstring out) {
    ldbg_record_filter f = filter_of(env, masks, scalars);
    ldbg_selection* sel = NULL;
    CHECK(query ? ldbg_graph_select_lookup(G(graph), &f, G(query), &sel) : ldbg_graph_select(G(graph), &f, &sel), NULL);
    int64_t n = 0, total = 0;
    ldbg_status st = ldbg_selection_count(sel, &n);
    if (st == LDBG_OK) st = ldbg_graph_info(G(query ? query : graph), NULL, NULL, NULL, &total, NULL);
    if (st == LDBG_OK && out) {
        jsize nc = (*env)->GetArrayLength(env, colours);
        jint* cols = (*env)->GetIntArrayElements(env, colours, NULL);
        const char* hp = headerPath ? (*env)->GetStringUTFChars(env, headerPath, NULL) : NULL;
        const char* op = (*env)->GetStringUTFChars(env, out, NULL);
        st = ldbg_selection_write_ctx(sel, (const int*)cols, (int)nc, hp, op);
        (*env)->ReleaseStringUTFChars(env, out, op);
        if (hp) (*env)->ReleaseStringUTFChars(env, headerPath, hp);
        (*env)->ReleaseIntArrayElements(env, colours, cols, JNI_ABORT);
    }
    if (st != LDBG_OK) { rethrow(env, st); ldbg_selection_free(sel); return NULL; }
    ldbg_selection_free(sel);
    jlong vals[2] = {n, total};
    jlongArray res = (*env)->NewLongArray(env, 2);
    if (res) (*env)->SetLongArrayRegion(env, res, 0, 2, vals);
    return res;
}
/* FindROIs(...).graph(): the selection opened as a resident graph without a file (ldbg_selection_open_graph); the handle is wrapped by
 * GpuCortexGraph.  The record numbers of a selection: ldbg_selection_indices. */
jlong JNIFN(GpuCortexTools, selectGraph)(JNIEnv* env, jclass c, jlong graph, jlongArray masks, jintArray scalars, jintArray colours) {
    ldbg_record_filter f = filter_of(env, masks, scalars);
    ldbg_selection* sel = NULL;
    CHECK(ldbg_graph_select(G(graph), &f, &sel), 0);
    jsize nc = (*env)->GetArrayLength(env, colours);
    jint* cols = (*env)->GetIntArrayElements(env, colours, NULL);
    ldbg_graph* g = NULL;
    ldbg_status st = ldbg_selection_open_graph(sel, (const int*)cols, (int)nc, NULL, &g);
    (*env)->ReleaseIntArrayElements(env, colours, cols, JNI_ABORT);
    ldbg_selection_free(sel);
    if (st != LDBG_OK) { rethrow(env, st); return 0; }
    return (jlong)(intptr_t)g;
}
jlongArray JNIFN(GpuCortexTools, selectIndices)(JNIEnv* env, jclass c, jlong graph, jlongArray masks, jintArray scalars) {
    ldbg_record_filter f = filter_of(env, masks, scalars);
    ldbg_selection* sel = NULL;
    CHECK(ldbg_graph_select(G(graph), &f, &sel), NULL);
    int64_t n = 0;
    ldbg_status st = ldbg_selection_count(sel, &n);
    int64_t* idx = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1));
    if (st == LDBG_OK) st = ldbg_selection_indices(sel, 0, n, idx);
    ldbg_selection_free(sel);
    jlongArray res = NULL;
    if (st == LDBG_OK) { res = (*env)->NewLongArray(env, (jsize)n); if (res) (*env)->SetLongArrayRegion(env, res, 0, (jsize)n, (const jlong*)idx); }
    free(idx);
    if (st != LDBG_OK) rethrow(env, st);
    return res;
}

/* ------------------------------------------------------------------ GpuCortexTools: RecoverExcludedKmers (ldbg_graph_recover)
 * RecoverExcludedKmers.java:29-108: the selection with a join, written as the reference's one-colour file.  Returns {numRecordsRecovered,
 * records written}; recoverGraph opens the same content as a resident graph without the file (ldbg_selection_open_recovered). */
jlongArray JNIFN(GpuCortexTools, recover)(JNIEnv* env, jclass c, jlong graph, jint childColor, jlong dirty, jstring out) {
    ldbg_selection* sel = NULL;
    int64_t recovered = 0, n = 0;
    CHECK(ldbg_graph_recover(G(graph), (int)childColor, G(dirty), &sel, &recovered), NULL);
    ldbg_status st = ldbg_selection_count(sel, &n);
    if (st == LDBG_OK && out) {
        const char* op = (*env)->GetStringUTFChars(env, out, NULL);
        st = ldbg_selection_write_recovered(sel, op);
        (*env)->ReleaseStringUTFChars(env, out, op);
    }
    ldbg_selection_free(sel);
    if (st != LDBG_OK) { rethrow(env, st); return NULL; }
    jlong vals[2] = {recovered, n};
    jlongArray res = (*env)->NewLongArray(env, 2);
    if (res) (*env)->SetLongArrayRegion(env, res, 0, 2, vals);
    return res;
}
jlong JNIFN(GpuCortexTools, recoverGraph)(JNIEnv* env, jclass c, jlong graph, jint childColor, jlong dirty) {
    ldbg_selection* sel = NULL;
    CHECK(ldbg_graph_recover(G(graph), (int)childColor, G(dirty), &sel, NULL), 0);
    ldbg_graph* g = NULL;
    ldbg_status st = ldbg_selection_open_recovered(sel, &g);
    ldbg_selection_free(sel);
    if (st != LDBG_OK) { rethrow(env, st); return 0; }
    return (jlong)(intptr_t)g;
}

/* ------------------------------------------------------------------ GpuCortexTools: sequences threaded through a graph (ldbg_graph_thread)
 * The inner loop of TrimPartitions.java:35-68, FilterPartitions.java:41-140, CountNovelKmersInPartitions.java:30-61, Coverage.java:29-47,
 * Call.loadChildWalk (Call.java:2358-2381) and Call.getRegions (:2425-2451).  graph or rois may be 0, not both; info receives
 * {sequences, windows, regions}.  The arrays a caller leaves null are not filled; the lengths of those given say how much is. */
#define T(h) ((ldbg_threading*)(intptr_t)(h))
static void null_pointer(JNIEnv* env, const char* what) {
    jclass c = (*env)->FindClass(env, "java/lang/NullPointerException");
    if (c) (*env)->ThrowNew(env, c, what);
}
jlong JNIFN(GpuCortexTools, thread)(JNIEnv* env, jclass c, jlong graph, jlong rois, jbyteArray bases, jlongArray offsets, jint flags, jlongArray info) {
    if (!bases || !offsets || !info) { null_pointer(env, "thread: bases, offsets and info must not be null"); return 0; }
    if ((*env)->GetArrayLength(env, info) < 3) { rethrow(env, LDBG_ERR_ARG); return 0; }
    jsize n = (*env)->GetArrayLength(env, offsets);
    jbyte* b = (*env)->GetByteArrayElements(env, bases, NULL);
    jlong* off = (*env)->GetLongArrayElements(env, offsets, NULL);
    ldbg_threading* t = NULL;
    int64_t v[3] = {0, 0, 0};
    ldbg_status st = ldbg_graph_thread(G(graph), G(rois), (const char*)b, (const int64_t*)off, n > 0 ? (int64_t)n - 1 : 0, (int)flags, &t);
    (*env)->ReleaseLongArrayElements(env, offsets, off, JNI_ABORT);
    (*env)->ReleaseByteArrayElements(env, bases, b, JNI_ABORT);
    if (st == LDBG_OK) st = ldbg_threading_info(t, &v[0], &v[1], &v[2], NULL);
    if (st != LDBG_OK) { if (t) ldbg_threading_free(t); rethrow(env, st); return 0; }
    jlong vals[3] = {(jlong)v[0], (jlong)v[1], (jlong)v[2]};
    (*env)->SetLongArrayRegion(env, info, 0, 3, vals);
    return (jlong)(intptr_t)t;
}
/* windows [first, first + n), n = the length of the first array given (all given arrays must be that long) */
void JNIFN(GpuCortexTools, threadWindows)(JNIEnv* env, jclass c, jlong threading, jlong first, jlongArray rec, jbyteArray info, jintArray copyIndex) {
    if (!rec && !info && !copyIndex) { null_pointer(env, "threadWindows: no output array"); return; }
    const jsize n = (*env)->GetArrayLength(env, rec ? (jarray)rec : info ? (jarray)info : (jarray)copyIndex);
    if ((info && (*env)->GetArrayLength(env, info) != n) || (copyIndex && (*env)->GetArrayLength(env, copyIndex) != n)) { rethrow(env, LDBG_ERR_ARG); return; }
    int64_t* r = rec ? (int64_t*)malloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1)) : NULL;
    uint8_t* i = info ? (uint8_t*)malloc((size_t)(n > 0 ? n : 1)) : NULL;
    int32_t* ci = copyIndex ? (int32_t*)malloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1)) : NULL;
    ldbg_status st = ldbg_threading_windows(T(threading), (int64_t)first, (int64_t)n, r, i, ci);
    if (st == LDBG_OK) {
        if (rec) (*env)->SetLongArrayRegion(env, rec, 0, n, (const jlong*)r);
        if (info) (*env)->SetByteArrayRegion(env, info, 0, n, (const jbyte*)i);
        if (copyIndex) (*env)->SetIntArrayRegion(env, copyIndex, 0, n, (const jint*)ci);
    }
    free(r); free(i); free(ci);
    if (st != LDBG_OK) rethrow(env, st);
}
/* sequences [firstSeq, firstSeq + n), n = firstHit.length; winStart holds n + 1 */
void JNIFN(GpuCortexTools, threadSummary)(JNIEnv* env, jclass c, jlong threading, jlong firstSeq, jlongArray winStart, jintArray firstHit, jintArray lastHit,
                                          jintArray numHits, jintArray numDistinct, jbyteArray ends) {
    if (!winStart || !firstHit || !lastHit || !numHits || !numDistinct || !ends) { null_pointer(env, "threadSummary: a null array"); return; }
    const jsize n = (*env)->GetArrayLength(env, firstHit);
    if ((*env)->GetArrayLength(env, winStart) != n + 1 || (*env)->GetArrayLength(env, lastHit) != n || (*env)->GetArrayLength(env, numHits) != n ||
        (*env)->GetArrayLength(env, numDistinct) != n || (*env)->GetArrayLength(env, ends) != n) { rethrow(env, LDBG_ERR_ARG); return; }
    const size_t m = (size_t)(n > 0 ? n : 1);
    int64_t* ws = (int64_t*)malloc(sizeof(int64_t) * (m + 1));
    int32_t* v = (int32_t*)malloc(sizeof(int32_t) * 4 * m);
    uint8_t* e = (uint8_t*)malloc(m);
    ldbg_status st = ldbg_threading_summary(T(threading), (int64_t)firstSeq, (int64_t)n, ws, v, v + m, v + 2 * m, v + 3 * m, e);
    if (st == LDBG_OK) {
        (*env)->SetLongArrayRegion(env, winStart, 0, n + 1, (const jlong*)ws);
        (*env)->SetIntArrayRegion(env, firstHit, 0, n, (const jint*)v);
        (*env)->SetIntArrayRegion(env, lastHit, 0, n, (const jint*)(v + m));
        (*env)->SetIntArrayRegion(env, numHits, 0, n, (const jint*)(v + 2 * m));
        (*env)->SetIntArrayRegion(env, numDistinct, 0, n, (const jint*)(v + 3 * m));
        (*env)->SetByteArrayRegion(env, ends, 0, n, (const jbyte*)e);
    }
    free(ws); free(v); free(e);
    if (st != LDBG_OK) rethrow(env, st);
}
/* regionOffsets: sequences + 1 entries; start and stop: the capacity, LDBG_ERR_CAPACITY when it is below the number of regions */
void JNIFN(GpuCortexTools, threadRegions)(JNIEnv* env, jclass c, jlong threading, jlongArray regionOffsets, jintArray start, jintArray stop) {
    if (!regionOffsets || !start || !stop) { null_pointer(env, "threadRegions: a null array"); return; }
    int64_t ns = 0;
    CHECK(ldbg_threading_info(T(threading), &ns, NULL, NULL, NULL), );
    const jsize cap = (*env)->GetArrayLength(env, start);
    if ((int64_t)(*env)->GetArrayLength(env, regionOffsets) != ns + 1 || (*env)->GetArrayLength(env, stop) != cap) { rethrow(env, LDBG_ERR_ARG); return; }
    int64_t* ro = (int64_t*)malloc(sizeof(int64_t) * (size_t)(ns + 1));
    int32_t* v = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)(cap > 0 ? cap : 1));
    ldbg_status st = ldbg_threading_regions(T(threading), ro, v, v + (cap > 0 ? cap : 1), (int64_t)cap);
    if (st == LDBG_OK) {
        const jsize nr = (jsize)ro[ns];
        (*env)->SetLongArrayRegion(env, regionOffsets, 0, (jsize)(ns + 1), (const jlong*)ro);
        (*env)->SetIntArrayRegion(env, start, 0, nr, (const jint*)v);
        (*env)->SetIntArrayRegion(env, stop, 0, nr, (const jint*)(v + (cap > 0 ? cap : 1)));
    }
    free(ro); free(v);
    if (st != LDBG_OK) rethrow(env, st);
}
void JNIFN(GpuCortexTools, threadFree)(JNIEnv* env, jclass c, jlong threading) { CHECK(ldbg_threading_free(T(threading)), ); }

/* ------------------------------------------------------------------ GpuTesserae: Tesserae.java:95-382 (ldbg_mosaic_align_batch, one problem)
 * paramBits: Double.doubleToRawLongBits of del, eps, rho, term; targets: the targets' bytes end to end, targetOffsets: targets + 1 entries.
 * Returns maxpath_copy, maxpath_state, maxpath_pos of the path, each `entries` long, one after the other; llkBits[0] = the bits of llk. */
jintArray JNIFN(GpuTesserae, alignNative)(JNIEnv* env, jclass c, jlongArray paramBits, jbyteArray query, jbyteArray targets, jlongArray targetOffsets, jlongArray llkBits) {
    if (!paramBits || !query || !targets || !targetOffsets || !llkBits) { null_pointer(env, "align: a null array"); return NULL; }
    if ((*env)->GetArrayLength(env, paramBits) != 4 || (*env)->GetArrayLength(env, llkBits) < 1 || (*env)->GetArrayLength(env, targetOffsets) < 1) { rethrow(env, LDBG_ERR_ARG); return NULL; }
    jlong* pb = (*env)->GetLongArrayElements(env, paramBits, NULL);
    ldbg_mosaic_params p;
    memcpy(&p, pb, sizeof(p));
    (*env)->ReleaseLongArrayElements(env, paramBits, pb, JNI_ABORT);
    const int64_t qoff[2] = {0, (int64_t)(*env)->GetArrayLength(env, query)};
    const int64_t tfirst[2] = {0, (int64_t)(*env)->GetArrayLength(env, targetOffsets) - 1};
    jbyte* q = (*env)->GetByteArrayElements(env, query, NULL);
    jbyte* t = (*env)->GetByteArrayElements(env, targets, NULL);
    jlong* off = (*env)->GetLongArrayElements(env, targetOffsets, NULL);
    ldbg_mosaic_result* r = NULL;
    ldbg_status st = ldbg_mosaic_align_batch(0, &p, 1, (const char*)q, qoff, tfirst, (const char*)t, (const int64_t*)off, &r);
    (*env)->ReleaseLongArrayElements(env, targetOffsets, off, JNI_ABORT);
    (*env)->ReleaseByteArrayElements(env, targets, t, JNI_ABORT);
    (*env)->ReleaseByteArrayElements(env, query, q, JNI_ABORT);
    if (st != LDBG_OK) { rethrow(env, st); return NULL; }
    int64_t n = 0, entries = 0, path_off[2] = {0, 0};
    uint8_t status = 0;
    double llk = 0;
    st = ldbg_mosaic_result_sizes(r, &n, &entries);
    if (st != LDBG_OK) { ldbg_mosaic_result_free(r); rethrow(env, st); return NULL; }
    int32_t* v = (int32_t*)malloc(sizeof(int32_t) * 3 * (size_t)(entries > 0 ? entries : 1));
    if (!v) {
        ldbg_mosaic_result_free(r);
        jclass oc = (*env)->FindClass(env, "java/lang/OutOfMemoryError");
        if (oc) (*env)->ThrowNew(env, oc, "Tesserae.align: the path arrays");
        return NULL;
    }
    const ldbg_mosaic_arrays a = {&status, &llk, path_off, v, v + entries, v + 2 * entries};
    st = ldbg_mosaic_result_get(r, &a);
    ldbg_mosaic_result_free(r);
    jintArray res = NULL;
    if (st == LDBG_OK && status != LDBG_OK) {
        free(v);
        jclass uc = (*env)->FindClass(env, "java/lang/UnsupportedOperationException");
        if (uc) (*env)->ThrowNew(env, uc, "Tesserae.align: a problem the device refuses (include/ldbg.h lists the cases)");
        return NULL;
    }
    if (st == LDBG_OK) {
        jlong bits;
        memcpy(&bits, &llk, sizeof(bits));
        (*env)->SetLongArrayRegion(env, llkBits, 0, 1, &bits);
        res = (*env)->NewIntArray(env, (jsize)(3 * entries));
        if (res) (*env)->SetIntArrayRegion(env, res, 0, (jsize)(3 * entries), (const jint*)v);
    }
    free(v);
    if (st != LDBG_OK) rethrow(env, st);
    return res;
}

/* ------------------------------------------------------------------ GpuSmithWaterman: SmithWaterman.java:89-294 (ldbg_sw_align_batch, one pair)
 * query, subject: the bytes after the header regex.  Returns SWResult.qseq then SWResult.sseq, each aligned_len bytes (:237-259 built
 * here from the columns and the filtered letters); scoreBits[0] = the bits of SWResult.score. */
jbyteArray JNIFN(GpuSmithWaterman, alignNative)(JNIEnv* env, jclass c, jbyteArray query, jbyteArray subject, jlongArray scoreBits) {
    if (!query || !subject || !scoreBits) { null_pointer(env, "align: a null array"); return NULL; }
    if ((*env)->GetArrayLength(env, scoreBits) < 1) { rethrow(env, LDBG_ERR_ARG); return NULL; }
    const int64_t qoff[2] = {0, (int64_t)(*env)->GetArrayLength(env, query)};
    const int64_t soff[2] = {0, (int64_t)(*env)->GetArrayLength(env, subject)};
    jbyte* q = (*env)->GetByteArrayElements(env, query, NULL);
    jbyte* s = (*env)->GetByteArrayElements(env, subject, NULL);
    ldbg_sw_result* r = NULL;
    ldbg_status st = ldbg_sw_align_batch(0, 1, (const char*)q, qoff, (const char*)s, soff, &r);
    (*env)->ReleaseByteArrayElements(env, subject, s, JNI_ABORT);
    (*env)->ReleaseByteArrayElements(env, query, q, JNI_ABORT);
    if (st != LDBG_OK) { rethrow(env, st); return NULL; }
    int64_t n = 0, ncols = 0, nq = 0, ns = 0;
    st = ldbg_sw_result_sizes(r, &n, &ncols, &nq, &ns);
    if (st != LDBG_OK) { ldbg_sw_result_free(r); rethrow(env, st); return NULL; }
    uint8_t status = 0;
    double score = 0;
    int32_t end_q = 0, end_s = 0, begin_q = 0, begin_s = 0, alen = 0;
    uint8_t* buf = (uint8_t*)malloc((size_t)(ncols + nq + ns + 1));
    if (!buf) {
        ldbg_sw_result_free(r);
        jclass oc = (*env)->FindClass(env, "java/lang/OutOfMemoryError");
        if (oc) (*env)->ThrowNew(env, oc, "SmithWaterman.align: the columns");
        return NULL;
    }
    uint8_t* cols = buf; uint8_t* ql = buf + ncols; uint8_t* sl = ql + nq;
    const ldbg_sw_arrays a = {&status, &score, &end_q, &end_s, &begin_q, &begin_s, &alen, NULL, NULL, cols, NULL, ql, NULL, sl};
    st = ldbg_sw_result_get(r, &a);
    ldbg_sw_result_free(r);
    if (st == LDBG_OK && status != LDBG_OK) {
        free(buf);
        jclass uc = (*env)->FindClass(env, "java/lang/UnsupportedOperationException");
        if (uc) (*env)->ThrowNew(env, uc, "SmithWaterman.align: a pair the device refuses (include/ldbg.h lists the cases)");
        return NULL;
    }
    jbyteArray res = NULL;
    if (st == LDBG_OK) {
        uint8_t* v = (uint8_t*)malloc((size_t)(2 * (int64_t)alen + 1));
        if (v) {
            uint8_t* a0 = v; uint8_t* a1 = v + alen;
            int64_t at = 0, x, y;
            if (end_q > 0) {
                for (y = 0; y < begin_s - 1; y++, at++) { a0[at] = '-'; a1[at] = sl[y]; }
                for (x = 0; x < begin_q - 1; x++, at++) { a0[at] = ql[x]; a1[at] = '-'; }
                x = begin_q - 1; y = begin_s - 1;
                for (int64_t k = 0; k < ncols; k++, at++) {
                    a0[at] = cols[k] == 1 ? (uint8_t)'-' : ql[x++];
                    a1[at] = cols[k] == 2 ? (uint8_t)'-' : sl[y++];
                }
                for (x = end_q; x < nq; x++, at++) { a0[at] = ql[x]; a1[at] = '-'; }
                for (y = end_s; y < ns; y++, at++) { a0[at] = '-'; a1[at] = sl[y]; }
            }
            jlong bits;
            memcpy(&bits, &score, sizeof(bits));
            (*env)->SetLongArrayRegion(env, scoreBits, 0, 1, &bits);
            res = (*env)->NewByteArray(env, (jsize)(2 * alen));
            if (res) (*env)->SetByteArrayRegion(env, res, 0, (jsize)(2 * alen), (const jbyte*)v);
            free(v);
        } else {
            jclass oc = (*env)->FindClass(env, "java/lang/OutOfMemoryError");
            if (oc) (*env)->ThrowNew(env, oc, "SmithWaterman.align: the aligned strings");
        }
    }
    free(buf);
    if (st != LDBG_OK) rethrow(env, st);
    return res;
}
