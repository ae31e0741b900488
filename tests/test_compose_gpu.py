"""The drop-in iterators stacked, in the product: every door on the device.  An operator iterator as the child of another
operator, statistic, writer or reducer hands down the doubles its pop() delivers (tests/compose_dropin.py, which
tests/test_compose_model.py runs over the emulated drop-in library); every stack is read once more with the matching
WTAMD_NO_DEVICE_*=1 and gives the same bits; the recorded stacks of the compiled reference (tests/golden/compose_fixtures.json)."""
import pytest

import compose_dropin as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def doors():
    from wiggletools_amd import _lib
    _lib.lib()
    return X.Doors(_lib.LIB_PATH)


@pytest.mark.parametrize("producer,length,n_chrom", X.CASES)
def test_every_consumer_over_a_stacked_producer(doors, oracle, tmp_path, monkeypatch, producer, length, n_chrom):
    """(a) the stacked child against the replay of its pops, (b) the exact model over those pops, and the host sweeps' bits."""
    failed = X.check_stack(doors, oracle, tmp_path, producer, length, n_chrom, setenv=monkeypatch.setenv)
    assert not failed, failed


@pytest.mark.parametrize("producer,length,n_chrom", [c for c in X.CASES if c[1] <= 3000])
def test_seek_through_a_stack(doors, producer, length, n_chrom):
    X.check_seek(doors, producer, length, n_chrom)


def test_the_recorded_stacks_of_the_compiled_reference(doors, oracle, monkeypatch):
    X.check_fixtures(doors, oracle, setenv=monkeypatch.setenv)


def test_both_feeder_routes_take_the_doubles(doors, oracle, tmp_path, monkeypatch):
    X.check_feeder_routes(doors, oracle, tmp_path, monkeypatch.setenv, monkeypatch.delenv)
