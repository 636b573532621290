"""bench.py's seed sampler (the draws of ngd_rmat_seeds against a vertex mask taken from the CSR shard)
gives the seeds of datagen.rmat_seeds, the sampler of the --full run and of the tests."""
import numpy as np
import pytest

import bench
from nebula_amd import datagen


@pytest.mark.parametrize("scale,ef", [(16, 1), (12, 16)])
def test_seed_sampler_equals_rmat_seeds(scale, ef):
    c = datagen.rmat_csr(scale, ef, 42, 10, with_in=True, threads=2)
    has_out = np.zeros(1 << scale, dtype=bool)
    for etype, off, _, _ in c.slots:
        if etype == datagen.RMAT_EDGE:
            has_out[c.vid[np.diff(off) > 0]] = True
    c.free()
    assert 0 < has_out.sum() < len(has_out)              # isolated vertices exist: the mask matters
    if ef == 1:                                          # so sparse that 1000 seeds take a second block of draws
        assert 1000 / has_out.mean() > 4 * 1000 + 64
    sample = bench.seed_sampler(np, scale, has_out)
    for sample_seed in (42, 43, 151):
        for k in (1, 20, 1000):
            want = [int(v) for v in datagen.rmat_seeds(scale, k, ef, 42, sample_seed, threads=2)]
            assert sample(sample_seed, k) == want
