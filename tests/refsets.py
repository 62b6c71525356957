"""Reference results shared by the GPU test files: a set's Dataset with the rows
and superReadIDs it must give, from the reference's goldens (fixtures) or from
the oracle (everything else), each computed once per run and never modified."""
import functools

from conftest import fixture_input, golden_rows, load_meta
from metagenomics_amd.overlap import Dataset, OverlapEngine
from oracle import OracleDataset, sorted_tuples


def super_dict(sup):
    """{str(ID): superReadID} of the contained reads, the form of the goldens' meta["super"]."""
    return {str(i): int(x) for i, x in enumerate(sup) if x}


def engine_with(opts):
    """A fresh context on device 0 with the options set."""
    e = OverlapEngine(0)
    for k, v in opts.items():
        e.set_option(k, v)
    return e


def from_oracle(seqs, l):
    """(Dataset, l, rows as sorted tuples, {id: superReadID}) of reads given as strings."""
    od = OracleDataset.from_strings(seqs, l)
    orows, osup, _, _ = od.overlaps(l)
    ds = Dataset.from_strings(seqs, l)
    assert ds.num_unique == od.num_unique
    return ds, l, sorted_tuples(orows), super_dict(osup)


@functools.lru_cache(maxsize=None)
def fixture_reference(name):
    """The same tuple for a reference-generated fixture."""
    meta = load_meta(name)
    return Dataset.from_files([fixture_input(name)], meta["l"]), meta["l"], golden_rows(name), meta["super"]


def first_unique_reads(codes, lens, l, n):
    """The first n unique reads (ID order) of a sampled set, as strings: a set of exactly n reads."""
    pool = Dataset.from_codes(codes, lens, l)
    assert pool.num_unique >= n
    return [pool.read(i) for i in range(1, n + 1)]
