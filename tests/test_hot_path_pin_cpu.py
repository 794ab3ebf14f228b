"""CPU (oracle backend): pipeline.run_hot_path and run_hot_path_samples on the reference's sample_h1 reads return the draft and the polished sequence the command line path
writes for them (hot_path_pin.py) - a recorded answer from another implementation of the flow, where the other tests of the two entry points compare one backend or one
entry point against the other through the same Python code."""
import pytest
import hot_path_pin as pin


@pytest.fixture(scope="module")
def single(oracle):
    return pin.check_single(oracle)


def test_run_hot_path_is_pinned(single):
    assert single["centers"][0][4] and "classify" not in single and "haplotypes" not in single


def test_run_hot_path_samples_is_pinned(oracle, single):
    pin.check_samples(oracle, single)
