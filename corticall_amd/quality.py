"""ComputeAssemblyQuality and the seed stage of ComputeInheritance over the device seed pass (ldbg_graph_variant_seeds).
No compute here beyond colour sets, the join's temporary file and formatting: the filter, the string graph and the walk from its starts
are HIP kernels, and so is the count that stands in for the aligner.

Mirrors  J/commands/quality/ComputeAssemblyQuality.java:44-61, 204-309
         J/commands/inheritance/ComputeInheritance.java:48-65, 238-404 (getVariantSeeds and its predicates; callVariants is not built)

Where the reference asks an aligner whether a k-mer has exactly one place in a reference (IndexedReference.find,
J/utils/io/reference/IndexedReference.java:90-101), the reference sequences are threaded through the graph and the windows that hit the
k-mer's record are counted, on either strand: a documented divergence (an exact count; what BWA reports for a multi-copy k-mer is not
pinned)."""
import math
import os
import tempfile

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


class ComputeInheritance:
    """The seed stage of ComputeInheritance (:48-60, getVariantSeeds :238-322).  references: dict draft sample name -> FASTA path or
    list of (name, sequence) — that draft's reference; parents: dict (its values are the sample names, as the reference's PARENTS map)
    or list of sample names; children: sample names; ref_name: the reference sample.  At most 8 drafts (the filter's unique entries)."""

    def __init__(self, graph, references, parents, children, ref_name):
        self.GRAPH, self.REFERENCES, self.CHILDREN, self.REF_NAME = graph, dict(references), list(children), ref_name
        self.PARENTS = list(parents.values()) if isinstance(parents, dict) else list(parents)

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

    def execute(self):
        raise NotImplementedError("ComputeInheritance.callVariants (ComputeInheritance.java:67-236) is not built: variant_seeds() is the seed stage")
