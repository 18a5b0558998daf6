package uk.ac.ox.well.cortexjdk.gpu;

import java.io.File;
import java.util.List;

/** Sort and Join on the device: commands/utils/Sort.java:20-49, commands/utils/Join.java:16-60 (over CortexCollection.java:218-293);
 *  FindROIs, the record prefilters and Remove over the device selection (ldbg_graph_select): commands/discover/roi/FindROIs.java:30-82,
 *  commands/prefilter/FindLowCoverage.java:32-67, FindDust.java:78-135, FindShared.java:41-118, commands/utils/Remove.java:29-86;
 *  RecoverExcludedKmers over the device selection with a join (ldbg_graph_recover): commands/discover/recover/RecoverExcludedKmers.java:29-108;
 *  contigs threaded through a graph (ldbg_graph_thread), the inner loop of commands/discover/call/TrimPartitions.java:35-68,
 *  FilterPartitions.java:41-140, CountNovelKmersInPartitions.java:30-61, commands/discover/display/Coverage.java:29-47, Call.loadChildWalk
 *  (Call.java:2358-2381) and Call.getRegions (:2425-2451). */
public final class GpuCortexTools {
    static { System.loadLibrary("ldbg_jni"); }
    private GpuCortexTools() {}

    /** the records of `in` in k-mer order under the rewritten header; returns the number of records */
    public static long sort(File in, File out) { return sort(in.getAbsolutePath(), out.getAbsolutePath(), 0); }

    /** the union of the k-mers of several sorted graphs, each graph's colours side by side */
    public static long join(List<File> ins, File out) {
        String[] paths = new String[ins.size()];
        for (int i = 0; i < paths.length; i++) { paths[i] = ins.get(i).getAbsolutePath(); }
        return join(paths, out.getAbsolutePath(), 0);
    }

    /** CortexGraphWriter over a selection: the header of `in` and its records `indices`, in that order (what FindTips writes) */
    public static void writeRecords(File in, long[] indices, File out) { writeRecords(in.getAbsolutePath(), indices, out.getAbsolutePath()); }

    public static int devices() { return deviceCount(); }

    /** TempLinksAssembler.buildLinks on the device: the links the reads of `sample` leave on `graph`, written to `out`; returns {k-mers with links, links} */
    public static long[] buildLinks(GpuCortexGraph graph, String sample, java.util.List<String> reads, File out) {
        java.io.ByteArrayOutputStream text = new java.io.ByteArrayOutputStream();
        long[] offsets = new long[reads.size() + 1];
        for (int i = 0; i < reads.size(); i++) {
            byte[] b = reads.get(i).getBytes(java.nio.charset.StandardCharsets.US_ASCII);
            text.write(b, 0, b.length);
            offsets[i + 1] = offsets[i] + b.length;
        }
        return buildLinks(graph.handle, sample, text.toByteArray(), offsets, out.getAbsolutePath());
    }

    private static long mask(java.util.Collection<Integer> colours) { long m = 0; for (int c : colours) { m |= 1L << c; } return m; }
    private static int[] range(int n) { int[] r = new int[n]; for (int i = 0; i < n; i++) { r[i] = i; } return r; }

    /** FindROIs: the k-mers the child has and no parent has, colour `child` alone under a fresh header; returns the number of novel records */
    public static long findROIs(GpuCortexGraph graph, java.util.Collection<Integer> parents, int child, File out) {
        return selectWrite(graph.handle, 0, new long[] { mask(parents), 1L << child, 0, 0 }, new int[] { -1, 0, -1, 0 }, new int[] { child }, null, out.getAbsolutePath())[0];
    }
    /** the same as a graph resident on the device, without a file: what Partition and an engine's rois(...) take */
    public static GpuCortexGraph findROIs(GpuCortexGraph graph, java.util.Collection<Integer> parents, int child) {
        return GpuCortexGraph.ofHandle(selectGraph(graph.handle, new long[] { mask(parents), 1L << child, 0, 0 }, new int[] { -1, 0, -1, 0 }, new int[] { child }));
    }
    /** record numbers of `graph` that pass a filter: masks {all_zero, all_positive, any_positive, none_positive}, scalars {cov_color, cov_below, degree_color, degree_above} */
    public static long[] select(GpuCortexGraph graph, long[] masks, int[] scalars) { return selectIndices(graph.handle, masks, scalars); }

    /** FindLowCoverage: writes the ROI records with coverage below minCoverage (the excluded ones); returns {numKept, numExcluded} */
    public static long[] findLowCoverage(GpuCortexGraph roi, File roiFile, int minCoverage, File out) {
        long[] r = selectWrite(roi.handle, 0, new long[4], new int[] { 0, minCoverage, -1, 0 }, range(roi.getNumColors()), roiFile.getAbsolutePath(), out.getAbsolutePath());
        return new long[] { r[1] - r[0], r[0] };
    }
    /** FindDust: writes the ROI records with more than 4 edges in colour 0; returns {numKept, numExcluded} */
    public static long[] findDust(GpuCortexGraph roi, File roiFile, File out) {
        long[] r = selectWrite(roi.handle, 0, new long[4], new int[] { -1, 0, 0, 4 }, range(roi.getNumColors()), roiFile.getAbsolutePath(), out.getAbsolutePath());
        return new long[] { r[1] - r[0], r[0] };
    }
    /** FindShared: writes the ROI records whose k-mer has coverage in a colour of `others` (not child, parent or ignored; not empty) of `graph`;
     *  NullPointerException for a ROI k-mer without a record in `graph`; returns {numKept, numExcluded} */
    public static long[] findShared(GpuCortexGraph graph, java.util.Collection<Integer> others, GpuCortexGraph roi, File roiFile, File out) {
        long[] r = selectWrite(graph.handle, roi.handle, new long[] { 0, 0, mask(others), 0 }, new int[] { -1, 0, -1, 0 }, range(roi.getNumColors()), roiFile.getAbsolutePath(), out.getAbsolutePath());
        return new long[] { r[1] - r[0], r[0] };
    }
    /** Remove: the records of the collection {primary, secondaries...} (its iterator view) without coverage in a secondary colour, reduced
     *  to the primary's colours under its header; returns {numKept, numRemoved} */
    public static long[] remove(File primary, List<File> secondaries, File out) {
        List<File> all = new java.util.ArrayList<>();
        all.add(primary);
        all.addAll(secondaries);
        GpuCortexGraph pg = new GpuCortexGraph(primary);
        int p = pg.getNumColors();
        pg.close();
        GpuCortexGraph cc = GpuCortexGraph.collection(all, false, 0);
        try {
            long sec = 0;
            for (int c = p; c < cc.getNumColors(); c++) { sec |= 1L << c; }
            long[] r = selectWrite(cc.handle, 0, new long[] { 0, 0, 0, sec }, new int[] { -1, 0, -1, 0 }, range(p), primary.getAbsolutePath(), out.getAbsolutePath());
            return new long[] { r[0], r[1] - r[0] };
        } finally {
            cc.close();
        }
    }

    private static int childColor(GpuCortexGraph graph, GpuCortexGraph dirty) {
        int childColor = graph.getColorForSampleName(dirty.getSampleName(0));
        if (childColor < 0) { throw new uk.ac.ox.well.cortexjdk.utils.exceptions.CortexJDKException("Sample '" + dirty.getSampleName(0) + "' not found in pedigree graph"); }
        return childColor;
    }
    /** RecoverExcludedKmers: the records of `graph` the child (dirty's sample 0) has, and those only another sample has whose k-mer `dirty`
     *  holds with coverage, patched with that coverage, written to `out` (one colour: colour 0's coverage and edge byte under the child's
     *  colour block, as the reference's writer leaves it); returns {numRecordsRecovered, records written} */
    public static long[] recoverExcludedKmers(GpuCortexGraph graph, GpuCortexGraph dirty, File out) {
        return recover(graph.handle, childColor(graph, dirty), dirty.handle, out.getAbsolutePath());
    }
    /** the same as a graph resident on the device, without a file */
    public static GpuCortexGraph recoverExcludedKmers(GpuCortexGraph graph, GpuCortexGraph dirty) {
        return GpuCortexGraph.ofHandle(recoverGraph(graph.handle, childColor(graph, dirty), dirty.handle));
    }

    public static final int THREAD_FIND_QUIRK = 1, THREAD_COPY_INDEX = 2;

    /** A batch of sequences threaded through `graph` and / or `rois` (either may be null, not both), held on the device until close().
     *  Windows are numbered through all sequences; sequence s owns [winStart[s], winStart[s + 1]). */
    public static final class Threading implements AutoCloseable {
        private long handle;
        public final long numSequences, numWindows, numRegions;
        Threading(long handle, long[] info) { this.handle = handle; numSequences = info[0]; numWindows = info[1]; numRegions = info[2]; }
        /** per window: rec (the record in `graph`, -1: none), info (bit 0 valid, 1 flipped, 2 palindrome, 3 in ROI), copyIndex (null unless asked for) */
        public void windows(long first, long[] rec, byte[] info, int[] copyIndex) { threadWindows(handle, first, rec, info, copyIndex); }
        /** per sequence, n = firstHit.length: winStart[n + 1], firstHit, lastHit (-1: none), numHits, numDistinct, ends (bit 0 / 1: first / last window in ROI) */
        public void summary(long firstSeq, long[] winStart, int[] firstHit, int[] lastHit, int[] numHits, int[] numDistinct, byte[] ends) {
            threadSummary(handle, firstSeq, winStart, firstHit, lastHit, numHits, numDistinct, ends);
        }
        /** Call.getRegions of every sequence: regionOffsets[numSequences + 1] into the inclusive pairs (start[i], stop[i]), numRegions of them */
        public void regions(long[] regionOffsets, int[] start, int[] stop) { threadRegions(handle, regionOffsets, start, stop); }
        @Override public void close() { if (handle != 0) { threadFree(handle); handle = 0; } }
    }

    public static Threading thread(GpuCortexGraph graph, GpuCortexGraph rois, java.util.List<String> seqs, int flags) {
        java.io.ByteArrayOutputStream text = new java.io.ByteArrayOutputStream();
        long[] offsets = new long[seqs.size() + 1];
        for (int i = 0; i < seqs.size(); i++) {
            byte[] b = seqs.get(i).getBytes(java.nio.charset.StandardCharsets.US_ASCII);
            text.write(b, 0, b.length);
            offsets[i + 1] = offsets[i] + b.length;
        }
        long[] info = new long[3];
        long h = thread(graph == null ? 0 : graph.handle, rois == null ? 0 : rois.handle, text.toByteArray(), offsets, flags, info);
        return new Threading(h, info);
    }

    private static native long thread(long graph, long rois, byte[] bases, long[] offsets, int flags, long[] info);
    private static native void threadWindows(long threading, long first, long[] rec, byte[] info, int[] copyIndex);
    private static native void threadSummary(long threading, long firstSeq, long[] winStart, int[] firstHit, int[] lastHit, int[] numHits, int[] numDistinct, byte[] ends);
    private static native void threadRegions(long threading, long[] regionOffsets, int[] start, int[] stop);
    private static native void threadFree(long threading);
    private static native long sort(String in, String out, int device);
    private static native long join(String[] ins, String out, int device);
    private static native void writeRecords(String in, long[] indices, String out);
    private static native int deviceCount();
    private static native long[] buildLinks(long graph, String sample, byte[] bases, long[] offsets, String out);
    private static native long[] selectWrite(long graph, long query, long[] masks, int[] scalars, int[] colours, String headerPath, String out);
    private static native long selectGraph(long graph, long[] masks, int[] scalars, int[] colours);
    private static native long[] selectIndices(long graph, long[] masks, int[] scalars);
    private static native long[] recover(long graph, int childColor, long dirty, String out);
    private static native long recoverGraph(long graph, int childColor, long dirty);
}
