package uk.ac.ox.well.cortexjdk.gpu;

/** utils/alignment/sw/SmithWaterman.java on the device (ldbg_sw_align_batch, one pair): Sequence.add, EDNAFULL.filter, the recurrences
 *  of :116-181, getMaxScorePos and the traceback run in the library; the header regex of :47-48 is applied here, and a char that is
 *  not ASCII goes over as '?', which filter turns into 'X' as it does the char itself. */
public final class GpuSmithWaterman {
    static { System.loadLibrary("ldbg_jni"); }

    /** SWResult: the two aligned strings and the score (-1 and empty strings where nothing is positive, :190-192) */
    public static final class Result {
        public final String qseq, sseq;
        public final double score;
        Result(String qseq, String sseq, double score) { this.qseq = qseq; this.sseq = sseq; this.score = score; }
    }

    private static byte[] pack(String s) {
        String t = s.replaceAll("^[\\s]*>[^\\r\\n]*[\\r\\n]+", "");
        byte[] b = new byte[t.length()];
        for (int i = 0; i < b.length; i++) { char c = t.charAt(i); b[i] = c < 128 ? (byte) c : (byte) '?'; }
        return b;
    }

    /** SmithWaterman.align(String, String) (:46-71) */
    public Result align(String qq, String ss) {
        long[] scoreBits = new long[1];
        byte[] v = alignNative(pack(qq), pack(ss), scoreBits);
        int n = v.length / 2;
        return new Result(new String(v, 0, n, java.nio.charset.StandardCharsets.ISO_8859_1), new String(v, n, n, java.nio.charset.StandardCharsets.ISO_8859_1),
                          Double.longBitsToDouble(scoreBits[0]));
    }

    /** :73-87 */
    public String[] getAlignment(String qq, String ss) {
        Result r = align(qq, ss);
        return new String[] { r.qseq, r.sseq };
    }

    private static native byte[] alignNative(byte[] query, byte[] subject, long[] scoreBits);
}
