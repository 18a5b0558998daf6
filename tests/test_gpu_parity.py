"""THE parity gate: every case of tests/parity_cases.py through the HIP library (libldbg.so, gfx950)
on a real MI355X, compared bit-exactly with the CPU oracle.  Run with `pytest -m gpu`."""
import pytest
import torch  # noqa: F401  (before libldbg: both bring a HIP runtime; torch's must be the one that initialises first)

from tests import parity_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import corticall_amd as ca
    l = ca.default_lib()
    assert l.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return l


def test_fixture_graph(orc, lib, tmp_path): pc.case_fixture_graph(orc, lib, tmp_path)


@pytest.mark.parametrize("k,ncol", [(5, 1), (21, 2), (31, 3), (32, 1), (33, 2), (47, 3), (63, 3), (64, 1), (65, 2), (95, 1)])
def test_random_find(orc, lib, tmp_path, k, ncol): pc.case_random_find(orc, lib, tmp_path, k, ncol)


@pytest.mark.parametrize("k", [32, 64, 96])
def test_all_bits_kmers(orc, lib, tmp_path, k): pc.case_all_bits_kmers(orc, lib, tmp_path, k)


def test_q1_tiny(orc, lib, tmp_path): pc.case_q1_tiny(orc, lib, tmp_path)
def test_unsorted_rejected(orc, lib, tmp_path): pc.case_unsorted_rejected(orc, lib, tmp_path)
def test_record_count_guard(orc, lib, tmp_path, monkeypatch): pc.case_record_count_guard(orc, lib, tmp_path, monkeypatch)
def test_rejected_open_frees_device_memory(lib, tmp_path): pc.case_rejected_open_frees_device_memory(lib, tmp_path)
def test_ref_short_contig_reconstruction(orc, lib, tmp_path): pc.test_ref_short_contig_reconstruction(orc, lib, tmp_path)
def test_ref_recruitment(orc, lib, tmp_path): pc.test_ref_recruitment(orc, lib, tmp_path)
def test_ref_cycles_without_and_with_links(orc, lib, tmp_path): pc.test_ref_cycles_without_and_with_links(orc, lib, tmp_path)
def test_ref_iterate_fwd_rev(orc, lib, tmp_path): pc.test_ref_iterate_fwd_rev(orc, lib, tmp_path)
def test_ref_go_forward_and_backward(orc, lib, tmp_path): pc.test_ref_go_forward_and_backward(orc, lib, tmp_path)
def test_ref_link_guided_walk(orc, lib, tmp_path): pc.test_ref_link_guided_walk(orc, lib, tmp_path)


@pytest.mark.parametrize("k,seed,links", [(9, 1, False), (9, 2, True), (21, 3, False), (31, 4, True), (47, 5, True), (63, 6, False), (33, 7, True), (32, 8, False), (64, 9, False), (65, 10, False)])
def test_random_walks(orc, lib, tmp_path, k, seed, links): pc.case_random_walks(orc, lib, tmp_path, k, seed, links)


@pytest.mark.parametrize("seed", range(8))
def test_dense_cycles(orc, lib, tmp_path, seed): pc.case_dense_cycles(orc, lib, tmp_path, seed)


@pytest.mark.parametrize("seed", range(10))
def test_run_steps(orc, lib, tmp_path, seed): pc.case_run_steps(orc, lib, tmp_path, seed)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5, 109, 231])      # (109: siblings that cut one stretch in different places, tools/soak_gpu.py; 231: a branch that opens INSIDE a stretch an ancestor crossed, tests/test_soak_hostsim.py)
def test_dfs_run_steps(orc, lib, tmp_path, seed): pc.case_dfs_run_steps(orc, lib, tmp_path, seed)


def test_long_walks(orc, lib, tmp_path): pc.case_long_walks(orc, lib, tmp_path)


def test_link_formats(orc, lib, tmp_path): pc.case_link_formats(orc, lib, tmp_path)


def test_sort(orc, lib, tmp_path): pc.case_sort(orc, lib, tmp_path)
def test_sort_rewrites_header(orc, lib, tmp_path): pc.case_sort_rewrites_header(orc, lib, tmp_path)
def test_join(orc, lib, tmp_path): pc.case_join(orc, lib, tmp_path)


def test_collection(orc, lib, tmp_path): pc.case_collection(orc, lib, tmp_path)


def test_ref_collection(orc, lib, tmp_path): pc.test_ref_collection(orc, lib, tmp_path)


def test_big_link_stores(orc, lib, tmp_path): pc.case_big_link_stores(orc, lib, tmp_path)


def test_hash_collision(orc, lib, tmp_path): pc.case_hash_collision(orc, lib, tmp_path)


@pytest.mark.parametrize("k,seed,links", [(9, 2, False), (21, 3, False), (31, 4, True), (47, 5, True)])
def test_dfs_rules(orc, lib, tmp_path, k, seed, links): pc.case_dfs_rules(orc, lib, tmp_path, k, seed, links)


@pytest.mark.parametrize("seed", range(4))
def test_dfs_dense(orc, lib, tmp_path, seed): pc.case_dfs_dense(orc, lib, tmp_path, seed)


def test_ref_dfs_with_sinks(orc, lib, tmp_path): pc.test_ref_dfs_with_sinks(orc, lib, tmp_path)
def test_ref_multiple_traversal_colors(orc, lib, tmp_path): pc.test_ref_multiple_traversal_colors(orc, lib, tmp_path)


def test_dfs_packed_results(orc, lib, tmp_path): pc.case_dfs_packed_results(orc, lib, tmp_path)


def test_dfs_second_launch_without_the_index(orc, lib, tmp_path, monkeypatch):
    """a search the run steps hand back sends its chunk round again without the run index: forced here, the results must not change"""
    monkeypatch.setenv("LDBG_DFS_FORCE_RETRY", "1")
    pc.case_dfs_run_steps(orc, lib, tmp_path, 0)
    pc.case_dfs_dense(orc, lib, tmp_path, 1)


def test_factory_validation(orc, lib, tmp_path): pc.case_factory_validation(orc, lib, tmp_path)


def test_ref_fill_gaps(orc, lib, tmp_path): pc.test_ref_fill_gaps(orc, lib, tmp_path)


@pytest.mark.parametrize("seed", range(3))
def test_fill_gaps_random(orc, lib, tmp_path, seed): pc.case_fill_gaps_random(orc, lib, tmp_path, seed)


@pytest.mark.parametrize("k,seed,links", [(21, 1, False), (31, 2, True), (47, 3, True)])
def test_partition(orc, lib, tmp_path, k, seed, links): pc.case_partition(orc, lib, tmp_path, k, seed, links)


@pytest.mark.parametrize("k,seed,links", [(21, 1, False), (31, 2, True), (47, 3, True), (32, 4, True)])
def test_findtips(orc, lib, tmp_path, k, seed, links): pc.case_findtips(orc, lib, tmp_path, k, seed, links)


@pytest.mark.parametrize("k,seed,links", [(21, 1, False), (31, 2, True), (47, 3, True), (32, 4, False)])
def test_facade(orc, lib, tmp_path, k, seed, links): pc.case_facade(orc, lib, tmp_path, k, seed, links)


def test_sharded_find_one_rank_rccl(orc, lib, tmp_path):
    """the exchange path of corticall_amd/distributed.py over RCCL with device buffers (one rank: this box has one GPU;
    the two-rank case runs on gloo in tests/test_distributed.py)"""
    import os
    import random
    import torch.distributed as dist
    from corticall_amd.distributed import ShardedCortexGraph
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29517")
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        rng = random.Random(2)
        p = str(tmp_path / "sh.ctx")
        orc.build_graph(p, [("a", [pc.rand_seq(rng, 3000)]), ("b", [pc.rand_seq(rng, 2000)])], 47)
        og = orc.Graph(p, tuned=True)
        sg = ShardedCortexGraph(p, lib=lib)
        kmers = [og.record_string(i).split()[0] for i in rng.sample(range(og.N), 500)]
        qs = [k if rng.random() < 0.5 else orc.revcomp(k) for k in kmers] + [pc.rand_seq(rng, 47) for _ in range(200)] + ["N" * 47]
        found, cov, edges, owner, lidx = sg.find_batch(qs)
        for i, q in enumerate(qs):
            eidx, ecov, eedges = og.find(q)
            assert bool(found[i]) == (eidx >= 0)
            if eidx >= 0:
                assert ecov == [int(c) for c in cov[i]] and eedges == [int(x) for x in edges[i]] and lidx[i] == eidx
        assert len(sg.find_batch([])[0]) == 0
        sg.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("k,with_links,ncol", [pytest.param(k, wl, 2, id="%d-%s" % (k, wl)) for k, wl in ((47, False), (47, True), (32, True), (63, True), (127, True), (96, False))]
                         + [(31, True, 5), (47, True, 32)])
def test_sharded_walks_one_rank_rccl(orc, lib, tmp_path, k, with_links, ncol):
    """walks over a sharded table's local image with device buffers and RCCL collectives, every call of a round queued on torch's
    stream (one rank here; two and three ranks on gloo in tests/test_distributed.py): link-guided and plain, odd and even k.
    ncol = 2: kid and mom.  ncol > 4: a family graph (parity_cases.family_haplotypes) with the kid at colour 0; "colour 1" of the
    configurations below is then the LAST colour, so image rows of 8 W + 5 C + ... bytes travel and colours beyond the packed word
    are walked"""
    pc.case_sharded_walks_one_rank_rccl(orc, lib, tmp_path, k, with_links, ncol)


@pytest.mark.parametrize("k,ncol", [pytest.param(k, 3, id=str(k)) for k in (21, 32, 127)] + [(32, 5), (31, 32)])
def test_sharded_dfs_one_rank_rccl(orc, lib, tmp_path, k, ncol):
    """dfs with stopping rules over a sharded table's local image on the device, RCCL collectives (one rank; two ranks on gloo in
    tests/test_distributed.py): DestinationStopper towards a sink, ExplorationStopper, and rules that consult a ROI graph.
    ncol = 3: kid, mom, dad, joining colours 1 and 2.  ncol > 4: further mutated copies behind them, the ROI graph what the kid
    alone has, joining colours C - 2 and C - 1"""
    pc.case_sharded_dfs_one_rank_rccl(orc, lib, tmp_path, k, ncol)


def test_dfs_step_limit(orc, lib, tmp_path, monkeypatch): pc.case_dfs_step_limit(orc, lib, tmp_path, monkeypatch)


def test_close_in_any_order(orc, lib, tmp_path): pc.case_close_in_any_order(orc, lib, tmp_path)


def test_small_visited_tables(orc, lib, tmp_path, monkeypatch):
    """visited tables that start at 64 entries: probe rounds wrap round the end of a table and tables regrow many times"""
    monkeypatch.setenv("LDBG_VT_INITIAL", "64")
    pc.case_long_walks(orc, lib, tmp_path)
    pc.case_dense_cycles(orc, lib, tmp_path, 2)
    pc.case_dfs_dense(orc, lib, tmp_path, 3)
    pc.case_dfs_rules(orc, lib, tmp_path, 31, 2, True)


def test_concurrent_engines(orc, lib, tmp_path): pc.case_concurrent_engines(orc, lib, tmp_path)


def test_lowercase_queries(orc, lib, tmp_path): pc.case_lowercase_queries(orc, lib, tmp_path)
