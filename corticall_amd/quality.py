"""ComputeAssemblyQuality and ComputeInheritance over the device seed pass (ldbg_graph_variant_seeds) and callVariant in
batches (ldbg_engine_variant_batch).  No compute here beyond colour sets, the grouping of seeds, the join's temporary
file, the float32 means of integer sums and formatting: the filter, the string graph, the walk from its starts, the three cursor loops of
a variant, the coverage sums and the alleles are HIP kernels, and so is the count that stands in for the aligner.

Mirrors  J/commands/quality/ComputeAssemblyQuality.java:44-61, 204-309
         J/commands/inheritance/ComputeInheritance.java:48-65, 238-404 (getVariantSeeds and its predicates)
         J/commands/inheritance/ComputeInheritance.java:67-236, 406-433 (callVariants, in the per-seed reading of DESIGN.md §18:
         call_variants(); execute(), the literal reading with its state shared between seeds, is not built)

Where the reference asks an aligner whether a k-mer has exactly one place in a reference (IndexedReference.find,
J/utils/io/reference/IndexedReference.java:90-101), the reference sequences are threaded through the graph and the windows that hit the
k-mer's record are counted, on either strand: a documented divergence (an exact count; what BWA reports for a multi-copy k-mer is not
pinned)."""
import math
import os
import tempfile

import numpy as np

from . import _native
from .contigs import _records
from .graph import CortexGraph
from .partition import Join


def java_int(v):
    """a sum kept in a Java int"""
    return ((int(v) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def java_quality(n_seeds, num_bases):
    """-10 * Math.log10((double) n / (double) b) -> (the double, the line println writes).  The last ulp of a JVM's log10 and the
    digits of Double.toString are not pinned: a finite value is written as Python's shortest repr."""
    n, b = float(n_seeds), float(num_bases)
    if b == 0.0:
        ratio = math.nan if n == 0.0 else math.copysign(math.inf, n)
    else:
        ratio = n / b
    if math.isnan(ratio) or ratio < 0:
        q = math.nan
    elif ratio == 0.0:
        q = math.inf
    elif math.isinf(ratio):
        q = -math.inf
    else:
        q = -10 * math.log10(ratio)
    text = "NaN" if math.isnan(q) else "Infinity" if q == math.inf else "-Infinity" if q == -math.inf else repr(q)
    return q, text


class ComputeAssemblyQuality:
    """ComputeAssemblyQuality.execute (:44-61): Q = -10 log10(good seeds / bases of the evaluated assembly's reference).  The two graphs
    are joined into one resident table (the reference reads them as a CortexCollection), eval is colour 0 and comp colour 1; a seed is
    a singly connected record with coverage in eval and none in comp whose k-mer occurs exactly once in eval_ref_fasta."""

    def __init__(self, eval_path, comp_path, eval_ref_fasta, out=None, device=0, lib=None):
        self.EVAL, self.COMP, self.REF, self.out, self.device = str(eval_path), str(comp_path), eval_ref_fasta, out, device
        self._lib = lib or _native.default_lib()
        self.n_seeds = self.n_unique = self.n_good = 0
        self.numBases = 0
        self.device_ms = 0.0

    def execute(self):
        """-> Q as a float; one line with it is written to `out`"""
        recs = _records(self.REF)
        fd, joined = tempfile.mkstemp(prefix="ldbg_quality_", suffix=".ctx")
        os.close(fd)
        try:
            Join([self.EVAL, self.COMP], joined, device=self.device, lib=self._lib).execute()
            g = CortexGraph(joined, device=self.device, lib=self._lib)
        finally:
            os.unlink(joined)
        try:
            with g.thread([s for _, s in recs]) as t, t.occurrences() as occ:
                with g.variant_seeds(all_zero=(1,), covered=[((0,), 1, 1)], unique=[(-1, occ)]) as seeds:
                    self.n_seeds, self.n_unique, self.n_good = seeds.n_seeds, seeds.n_unique, seeds.n_good
                    self.device_ms = seeds.device_ms + occ.device_ms
        finally:
            g.close()
        self.numBases = java_int(sum(len(s) for _, s in recs))
        q, text = java_quality(self.n_good, self.numBases)
        if self.out is not None:
            with open(self.out, "w", newline="") as f:
                f.write(text + "\n")
        return q


VARIANT_TYPES = ("SNP", "MNP", "DEL", "INS")      # :187-197, the first rule that applies


def variant_mean(total, flagged, n, coverages=None):
    """(int) (sum / (float) n) of a float that had the vertices' coverages added to it in order (ComputeInheritance.java:170-174,
    :202-206).  total: the exact integer sum; while the magnitudes add up to less than 2^24 (not flagged) every partial sum is an
    integer a float holds, so the float sum is float32(total).  A flagged sum is redone in order: coverages() -> the Java ints."""
    if not flagged:
        return int(np.float32(np.float32(int(total)) / np.float32(int(n))))
    acc = np.float32(0.0)
    for v in coverages():
        acc = np.float32(acc + np.float32(int(v)))
    return int(np.float32(acc / np.float32(int(n))))


def _kmer_ascii(words, k):
    """packed k-mers u64[n, W] -> their text as u8[n, k]"""
    n, W = words.shape
    out = np.empty((n, k), dtype=np.uint8)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    for p in range(k):
        off = 2 * (k - 1 - p)
        out[:, p] = bases[((words[:, W - 1 - off // 64] >> np.uint64(off % 64)) & np.uint64(3)).astype(np.int64)]
    return out


def table_text(entries):
    """TableWriter (J/utils/io/table/TableWriter.java:37-52): the header from the first entry's keys, fields separated by tabs, a field
    a later entry lacks written NA, a key the header lacks dropped, every line ended by \\n; no entry: nothing"""
    if not entries:
        return ""
    header = list(entries[0])
    return "".join("\t".join(row) + "\n" for row in [header] + [[e.get(h, "NA") for h in header] for e in entries])


class ComputeInheritance:
    """ComputeInheritance: the seed stage (:48-60, getVariantSeeds :238-322) and callVariants (:67-236) in its per-seed reading.  references: dict draft sample name -> FASTA path or
    list of (name, sequence) — that draft's reference; parents: dict (its values are the sample names, as the reference's PARENTS map)
    or list of sample names; children: sample names; ref_name: the reference sample.  At most 8 drafts (the filter's unique entries)."""

    def __init__(self, graph, references, parents, children, ref_name):
        self.GRAPH, self.REFERENCES, self.CHILDREN, self.REF_NAME = graph, dict(references), list(children), ref_name
        self.PARENTS = list(parents.values()) if isinstance(parents, dict) else list(parents)
        self.PARENT_NAMES = dict(parents) if isinstance(parents, dict) else {}      # the PARENTS map itself: its keys name the columns' values
        self.n_variants = self.n_no_other_parent = 0
        self.status_counts = {}
        self.device_ms = 0.0

    def colours(self):
        """-> (ref colour, parent colours, draft colours, child colours of the filter): :50-53 and getChildColors :324-336"""
        g = self.GRAPH
        ref = g.getColorForSampleName(self.REF_NAME)
        parents = sorted(set(g.getColorsForSampleNames(self.PARENTS)))
        drafts = sorted(set(g.getColorsForSampleNames(list(self.REFERENCES))))
        ignore = set(parents) | set(drafts) | {ref}
        return ref, parents, drafts, [c for c in range(g.getNumColors()) if c not in ignore]

    def variant_seeds(self):
        """-> the selection of good seeds (n_seeds, n_unique, n_good as the reference logs them)"""
        g = self.GRAPH
        _, parents, drafts, children = self.colours()
        nothing = ((0,), 1, 0)                      # at_least > at_most: a clause no record passes
        covered = [(parents, 1, 1) if parents else nothing, (drafts, 1, 1) if drafts else nothing]       # isSharedWithOnlyOneParent :338-350
        if len(children) != 1:                                                                           # isSharedWithSomeChildren :352-370
            covered.append((children, 2, len(children) - 1) if children else nothing)
        by_colour = {g.getColorForSampleName(name): ref for name, ref in self.REFERENCES.items()}
        held = []
        try:
            unique = []
            for c in drafts:                        # hasUniqueCoordinates :385-404: the one covered draft's reference
                t = g.thread([s for _, s in _records(by_colour[c])])
                held.append(t)
                occ = t.occurrences()
                held.append(occ)
                unique.append((c, occ))
            return g.variant_seeds(covered=covered, unique=unique)
        finally:
            for x in reversed(held):
                x.close()

    def call_variants(self, coordinates=None, out=None, max_steps=None):
        """callVariants (:67-236) with every seed called on its own: the child's walks traverse the child's colour alone and the
        parent's walk the colour of the parent that does not share the child's allele.  coordinates: a FASTA path or a
        list of (name, sequence), None: REFERENCES["ref"] (:167-168); where the reference asks its aligner for the places of source and
        destination, the sequences are threaded through the graph and the occurrences counted.  -> the entries (dicts of strings, keys
        in the reference's order) in (chrom, pos) order; written to `out` as TableWriter writes them."""
        from .traversal import ContigStopper, TraversalEngineFactory, profile_get
        from .traversal_utils import java_string_set_order
        g = self.GRAPH
        if coordinates is None:
            if "ref" not in self.REFERENCES:
                raise KeyError('call_variants: no coordinates given and REFERENCES has no "ref" entry (ComputeInheritance.java:167)')
            coordinates = self.REFERENCES["ref"]
        recs = _records(coordinates)
        _, parents, _, _ = self.colours()
        child_cols = sorted(set(g.getColorsForSampleNames(self.CHILDREN)))
        k = g.getKmerSize()
        ms0 = profile_get("variants", g._lib)[0] + profile_get("cursor", g._lib)[0]
        self.n_variants = self.n_no_other_parent = 0
        self.status_counts = {}
        # the seeds' records, gathered on the device (the selection as a table of its own): k-mer text and coverages of the seeds alone
        with self.variant_seeds() as sel:
            seeds = np.asarray(sel.indices(), dtype=np.int64)
            words = np.zeros((0, g.getKmerBits()), dtype=np.uint64)
            cov = np.zeros((0, g.getNumColors()), dtype=np.int32)
            if sel.count:
                picked = sel.graph(list(range(g.getNumColors())))
                try:
                    words, cov, _ = picked.records(0, sel.count)
                finally:
                    picked.close()
        text = _kmer_ascii(words, k)
        # per seed the parent that shares the child's allele and the one that does not (:109-117), then the (seed, child colour) items
        share, other = np.full(len(seeds), -1), np.full(len(seeds), -1)
        for pc in parents:
            share[cov[:, pc] > 0] = pc
            other[cov[:, pc] == 0] = pc
        self.n_no_other_parent = int((other < 0).sum())
        groups = {}
        for i in np.nonzero(other >= 0)[0]:
            for c in child_cols:
                if cov[i, c] > 0:
                    groups.setdefault((c, int(other[i])), []).append(int(i))
        engines = {}

        def engine(colour):
            if colour not in engines:
                engines[colour] = TraversalEngineFactory(lib=g._lib).traversalColors(colour).graph(g).stoppingRule(ContigStopper).make()
            return engines[colour]

        called = {}                                      # seed -> (child colour, fields of its call): the first child colour that calls
        tried = {}
        try:
            for (c, p) in sorted(groups):
                idx = groups[(c, p)]
                r = engine(c).variant_batch(engine(p), text[idx], p, child_cols, max_steps)
                ao, raw = r["allele_offsets"], r["alleles"].tobytes().decode()
                redo = {j: q for q, j in enumerate(j for j in range(len(idx)) if r["status"][j] == 0 and (r["child_flag"][j].any() or r["parent_flag"][j]))}
                contigs = engine(c).variant_batch(engine(p), text[[idx[j] for j in redo]], p, child_cols, max_steps, contigs=True) if redo else None
                for j, i in enumerate(idx):
                    if i in called:
                        continue
                    tried[i] = int(r["status"][j])
                    if tried[i] != 0:
                        continue
                    vertices = None
                    if j in redo:                        # a flagged sum: the coverages of the seed's two contigs, one lookup per contig
                        q = redo[j]
                        cw = contigs["child_words"][contigs["child_offsets"][q]:contigs["child_offsets"][q + 1]]
                        pw = contigs["parent_words"][contigs["parent_offsets"][q]:contigs["parent_offsets"][q + 1]]
                        vertices = (g.find_batch(_kmer_ascii(cw, k))[1], g.find_batch(_kmer_ascii(np.concatenate([cw[:1], pw]), k))[1])
                    in_order = lambda covs, colour: (lambda: covs[:, colour].tolist())
                    means = [variant_mean(r["child_sum"][j, m], r["child_flag"][j, m], r["n_child"][j], in_order(vertices[0], cc) if vertices else None)
                             for m, cc in enumerate(child_cols)]
                    called[i] = dict(c=c, p=p, source=int(r["source_rec"][j]), dest=int(r["dest_rec"][j]), type=VARIANT_TYPES[int(r["type"][j])],
                                     cov_parent=variant_mean(r["parent_sum"][j], r["parent_flag"][j], r["n_parent"][j], in_order(vertices[1], p) if vertices else None),
                                     means=means, alleles=raw[ao[2 * j]:ao[2 * j + 1]] + "/" + raw[ao[2 * j + 1]:ao[2 * j + 2]])
        finally:
            for e in engines.values():
                e.close()
        for st in tried.values():
            self.status_counts[st] = self.status_counts.get(st, 0) + 1
        # coordinates: source and destination each once in the reference, on one sequence
        entries = {}
        if called:
            names = java_string_set_order(list(self.PARENT_NAMES))
            with g.thread([s for _, s in recs]) as t, t.occurrences() as occ:
                count = occ.count
                want = sorted({v["source"] for v in called.values()} | {v["dest"] for v in called.values()})
                once = [x for x in want if count[x] == 1]
                place = dict(zip(once, occ.positions(once)))
            for i in sorted(called):                     # ascending record order: a later seed replaces an earlier one at its place
                v = called[i]
                if v["source"] not in place or v["dest"] not in place or place[v["source"]][0] != place[v["dest"]][0]:
                    continue
                seq, offset, _ = place[v["source"]]
                fields = recs[seq][0].split()
                te = {"chrom": fields[0] if fields else "", "pos": str(offset + 1), "type": v["type"], "cov_parent": str(v["cov_parent"])}
                for m, cc in enumerate(child_cols):
                    pc = v["p"] if cov[i, cc] == 0 else int(share[i])
                    sample = g.getSampleName(pc) if pc >= 0 else None
                    for ref_name in names:
                        if self.PARENT_NAMES[ref_name] == sample:
                            te[g.getSampleName(cc)] = "%s:%d" % (ref_name, v["means"][m])
                            break
                te["alleles"] = v["alleles"]
                entries[(te["chrom"], offset + 1)] = te
                self.n_variants += 1
        result = [entries[key] for key in sorted(entries)]
        self.device_ms = profile_get("variants", g._lib)[0] + profile_get("cursor", g._lib)[0] - ms0
        if out is not None:
            with open(out, "w", newline="") as f:
                f.write(table_text(result))
        return result

    def execute(self):
        raise NotImplementedError("ComputeInheritance.callVariants (ComputeInheritance.java:67-236) as the reference runs it, with the engines' colours "
                                  "shared between seeds, is not built (DESIGN.md §18): call_variants() calls every seed on its own")

