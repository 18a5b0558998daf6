package uk.ac.ox.well.cortexjdk.gpu;

import java.util.ArrayList;
import java.util.List;
import java.util.Map;

/** utils/alignment/mosaic/Tesserae.java on the device (ldbg_mosaic_align_batch): the recurrences and the traceback of alignAll
 *  (:188-382) run there; the text tracks of :385-492 and toString (:512-545) are built here from maxpath_copy / _state / _pos.
 *  A track is {name, text, start, end} as the reference's Triple&lt;String, String, Pair&lt;Integer, Integer&gt;&gt;. */
public final class GpuTesserae {
    static { System.loadLibrary("ldbg_jni"); }

    /** one entry of align's list */
    public static final class Track {
        public final String name, text;
        public final int start, end;
        Track(String name, String text, int start, int end) { this.name = name; this.text = text; this.start = start; this.end = end; }
    }

    private final double del, eps, rho, term;
    private double llk;
    private String editTrack;
    private List<Track> path = new ArrayList<>();

    public GpuTesserae() { this(0.025, 0.75, 0.0001, 0.001); }
    public GpuTesserae(double del, double eps, double rho, double term) { this.del = del; this.eps = eps; this.rho = rho; this.term = term; }

    /** Tesserae.align (:95-103); the targets in the map's iteration order */
    public List<Track> align(String query, Map<String, String> targets) {
        List<String> names = new ArrayList<>();
        List<String> seqs = new ArrayList<>();
        names.add("query");
        seqs.add(query);
        java.io.ByteArrayOutputStream text = new java.io.ByteArrayOutputStream();
        long[] offsets = new long[targets.size() + 1];
        int t = 0;
        for (Map.Entry<String, String> e : targets.entrySet()) {
            names.add(e.getKey());
            seqs.add(e.getValue());
            byte[] b = e.getValue().getBytes(java.nio.charset.StandardCharsets.ISO_8859_1);
            text.write(b, 0, b.length);
            offsets[t + 1] = offsets[t] + b.length;
            t++;
        }
        long[] bits = { Double.doubleToRawLongBits(del), Double.doubleToRawLongBits(eps), Double.doubleToRawLongBits(rho), Double.doubleToRawLongBits(term) };
        long[] llkBits = new long[1];
        int[] v = alignNative(bits, query.getBytes(java.nio.charset.StandardCharsets.ISO_8859_1), text.toByteArray(), offsets, llkBits);
        llk = Double.longBitsToDouble(llkBits[0]);
        int n = v.length / 3;
        path = new ArrayList<>();

        // :396-409
        StringBuilder sb = new StringBuilder();
        int posStart = -1, posEnd = -1, posTarget = 1;
        for (int i = 0; i < n; i++) {
            if (v[n + i] == 3) { sb.append("-"); }
            else {
                if (posStart == -1) { posStart = posTarget - 1; }
                posEnd = posTarget - 1;
                sb.append(query.charAt(posTarget - 1));
                posTarget++;
            }
        }
        path.add(new Track(names.get(0), sb.toString(), posStart, posEnd));

        // :412-430
        sb = new StringBuilder();
        posTarget = 1;
        for (int i = 0; i < n; i++) {
            if (v[n + i] == 1) {
                sb.append(query.charAt(posTarget - 1) == seqs.get(v[i] - 1).charAt(v[2 * n + i] - 1) ? "|" : " ");
                posTarget++;
            } else if (v[n + i] == 2) {
                posTarget++;
                sb.append("^");
            } else {
                sb.append("~");
            }
        }
        editTrack = sb.toString();

        // :440-492
        String currentTrack = names.get(v[0] - 1);
        sb = new StringBuilder();
        posStart = -1;
        posEnd = -1;
        int lastKnownPos = -1;
        boolean uppercase = true;
        for (int i = 0; i < n; i++) {
            int before = i > 0 ? v[2 * n + i - 1] : 0;
            if (i > 0 && v[i] == v[i - 1] && Math.abs(v[2 * n + i] - v[2 * n + i - 1]) > 1 || v[2 * n + i] == lastKnownPos + 1) {
                path.add(new Track(currentTrack, sb.toString(), posStart, posEnd));
                uppercase = !uppercase;
                lastKnownPos = before;
                if (posStart != posEnd) { posStart = v[2 * n + i] - 1; posEnd = v[2 * n + i] - 1; }
                currentTrack = names.get(v[i] - 1);
                sb = new StringBuilder();
                for (int s = 0; s < i; s++) { sb.append(' '); }
            }
            if (i > 0 && v[i] != v[i - 1]) {
                path.add(new Track(currentTrack, sb.toString(), posStart, posEnd));
                uppercase = true;
                if (posStart != posEnd) { posStart = v[2 * n + i] - 1; posEnd = v[2 * n + i] - 1; }
                currentTrack = names.get(v[i] - 1);
                sb = new StringBuilder();
                for (int s = 0; s < i; s++) { sb.append(' '); }
            }
            if (v[n + i] == 2) { sb.append("-"); }
            else {
                char ch = seqs.get(v[i] - 1).charAt(v[2 * n + i] - 1);
                ch = uppercase ? Character.toUpperCase(ch) : Character.toLowerCase(ch);
                if (posStart == -1) { posStart = v[2 * n + i] - 1; }
                posEnd = v[2 * n + i] - 1;
                sb.append(ch);
            }
        }
        path.add(new Track(currentTrack, sb.toString(), posStart, posEnd));
        return path;
    }

    public double getMaximumLogLikelihood() { return llk; }
    public String getEditTrack() { return editTrack; }

    /** Tesserae.toString (:512-545) */
    @Override
    public String toString() {
        int maxNameLength = 0;
        for (Track t : path) { maxNameLength = Math.max(maxNameLength, String.format("%s (%d-%d)", t.name, t.start, t.end).length()); }
        String format = "%" + maxNameLength + "s";
        StringBuilder sb = new StringBuilder();
        for (int i = 0; i < path.size(); i++) {
            Track t = path.get(i);
            sb.append(String.format(format, String.format("%s (%d-%d)", t.name, t.start, t.end))).append(" ").append(t.text).append("\n");
            if (i == 0) { sb.append(String.format(format, " ")).append(" ").append(editTrack).append("\n"); }
        }
        sb.append("\n").append("Mllk: ").append(llk).append("\n");
        return sb.toString();
    }

    private static native int[] alignNative(long[] paramBits, byte[] query, byte[] targets, long[] targetOffsets, long[] llkBits);
}
