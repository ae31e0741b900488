"""The drop-in iterators stacked, in the emulated drop-in library (tests/emu/build.py: csrc/wt_iter_abi.cpp without the HIP
units, so every door sweeps on the host): an operator iterator as the child of another operator, statistic, writer or reducer
must hand down the doubles its pop() delivers (tests/compose_dropin.py, which tests/test_compose_gpu.py runs over the product),
and the recorded stacks of the compiled reference (tests/golden/compose_fixtures.json)."""
import pytest

import compose_dropin as X


@pytest.fixture(scope="module")
def doors():
    from emu import build as emu_build
    return X.Doors(emu_build.build_dropin())


@pytest.mark.parametrize("producer,length,n_chrom", X.CASES)
def test_every_consumer_over_a_stacked_producer(doors, oracle, tmp_path, producer, length, n_chrom):
    """(a) the stacked child against the replay of its pops and (b) the exact model over those pops, consumer by consumer."""
    failed = X.check_stack(doors, oracle, tmp_path, producer, length, n_chrom)
    assert not failed, failed


@pytest.mark.parametrize("producer,length,n_chrom", [c for c in X.CASES if c[1] <= 3000])
def test_seek_through_a_stack(doors, producer, length, n_chrom):
    X.check_seek(doors, producer, length, n_chrom)


def test_the_recorded_stacks_of_the_compiled_reference(doors, oracle):
    """tests/golden/compose_fixtures.json: the reference hands doubles down a stack, and so do the stacked iterators."""
    X.check_fixtures(doors, oracle)


def test_both_feeder_routes_take_the_doubles(doors, oracle, tmp_path, monkeypatch):
    X.check_feeder_routes(doors, oracle, tmp_path, monkeypatch.setenv, monkeypatch.delenv)
