"""Graph construction (ldbg_graph_build): sequences of an ordered list of samples -> the sorted multi-colour graph,
built on the device as TempGraphAssembler.buildGraph (J/utils/assembler/TempGraphAssembler.java:19-127) builds it on the host.
No compute here: this module marshals the sequences and reads FASTA text."""
import ctypes as C
import os

import numpy as np

from . import _native

SPLIT_NON_ACGT = 1      # LDBG_BUILD_SPLIT_NON_ACGT


def _marshal(samples):
    """samples: dict name -> sequences, or list of (name, sequences); sequences: list of str / bytes -> (ldbg_build_sample[], n, keep-alive)"""
    items = list(samples.items()) if isinstance(samples, dict) else [(n, s) for n, s in samples]
    arr = (_native.BuildSample * max(1, len(items)))()
    keep = []
    for i, (name, seqs) in enumerate(items):
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        text = np.frombuffer(b"".join(bs) or b"\0", dtype=np.uint8)
        offs = np.zeros(len(bs) + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(b) for b in bs], dtype=np.int64)
        nm = name.encode() if isinstance(name, str) else bytes(name)
        keep += [text, offs, nm]
        arr[i].sample_name = nm
        arr[i].bases = text.ctypes.data
        arr[i].offsets = offs.ctypes.data
        arr[i].n_sequences = len(bs)
    return arr, len(items), keep


def build_ctx(samples, k, path, device=0, split_non_acgt=False, lib=None):
    """the graph of `samples` written to `path` (ldbg_graph_build_ctx) -> number of records"""
    lib = lib or _native.default_lib()
    arr, n, keep = _marshal(samples)
    nrec = C.c_int64()
    lib.check(lib.dll.ldbg_graph_build_ctx(arr, n, int(k), SPLIT_NON_ACGT if split_non_acgt else 0, int(device), os.fsencode(str(path)), C.byref(nrec)))
    del keep
    return nrec.value


def build_graph(samples, k, device=0, path=None, split_non_acgt=False, lib=None):
    """CortexGraph.build: the resident graph of `samples` (ldbg_graph_build); with `path` the file is written (one build, the records
    downloaded once) and opened"""
    from .graph import CortexGraph
    lib = lib or _native.default_lib()
    if path is not None:
        build_ctx(samples, k, path, device, split_non_acgt, lib)
        return CortexGraph(path, device=device, lib=lib)
    arr, n, keep = _marshal(samples)
    h = C.c_void_p()
    lib.check(lib.dll.ldbg_graph_build(arr, n, int(k), SPLIT_NON_ACGT if split_non_acgt else 0, int(device), C.byref(h)))
    del keep
    g = CortexGraph._from_handle(h, lib, "<build>")
    g._borrowed = False
    return g


def _marshal_reads(reads):
    """list of str / bytes -> (the reads back to back as uint8, their n + 1 offsets as int64)"""
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in reads]
    text = np.frombuffer(b"".join(bs) or b"\0", dtype=np.uint8)
    offs = np.zeros(len(bs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(x) for x in bs], dtype=np.int64)
    return text, offs


def build_links_ctp(graph, sample, reads, path, lib=None):
    """the links the reads of `sample` leave on the open graph, written to `path` as TempLinksAssembler.buildLinks writes them
    (ldbg_links_build_ctp) -> (k-mers with links, links)"""
    lib = lib or graph._lib
    text, offs = _marshal_reads(reads)
    nk, nl = C.c_int64(), C.c_int64()
    nm = sample.encode() if isinstance(sample, str) else bytes(sample)
    lib.check(lib.dll.ldbg_links_build_ctp(graph._h, nm, C.c_void_p(text.ctypes.data), C.c_void_p(offs.ctypes.data), C.c_int64(len(offs) - 1), 0,
                                           os.fsencode(str(path)), C.byref(nk), C.byref(nl)))
    return nk.value, nl.value


def read_fasta(path):
    """the sequences of a plain-text FASTA: '>' lines separate them, the lines between are joined"""
    seqs, cur = [], None
    with open(path, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                if cur is not None:
                    seqs.append(b"".join(cur))
                cur = []
            elif line.strip():
                if cur is None:
                    cur = []
                cur.append(line.strip())
    if cur is not None:
        seqs.append(b"".join(cur))
    return seqs


class Build:
    """the graph of one plain-text FASTA per sample, written to `out`.  fastas: dict sample -> path, or list of (sample, path).  Bytes
    other than ACGTacgt (runs of N) cut their sequence in two — LDBG_BUILD_SPLIT_NON_ACGT, an extension: the reference's builder
    throws on such a byte."""

    def __init__(self, fastas, k, out, device=0, lib=None):
        self.fastas = list(fastas.items()) if isinstance(fastas, dict) else [(n, p) for n, p in fastas]
        self.k, self.out, self.device = int(k), str(out), device
        self._lib = lib or _native.default_lib()

    def execute(self):
        """-> number of records written"""
        samples = [(name, read_fasta(p)) for name, p in self.fastas]
        return build_ctx(samples, self.k, self.out, self.device, True, self._lib)


class BuildLinks:
    """the links of a plain-text FASTA of reads of `sample` on the open graph, written to `out`"""

    def __init__(self, graph, sample, fasta, out, lib=None):
        self.graph, self.sample, self.fasta, self.out = graph, sample, fasta, str(out)
        self._lib = lib or graph._lib

    def execute(self):
        """-> (k-mers with links, links)"""
        return build_links_ctp(self.graph, self.sample, read_fasta(self.fasta), self.out, lib=self._lib)
