"""GPU: the pin of test_hot_path_pin_cpu.py on the HIP library - pipeline.run_hot_path and run_hot_path_samples on the reference's sample_h1 reads (274 reads of at most
725 bases) return the recorded draft and polished sequence of the command line path (hot_path_pin.py)."""
import pytest
import hot_path_pin as pin

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def single(gpu_api):
    return pin.check_single(gpu_api)


def test_run_hot_path_is_pinned(single):
    assert single["centers"][0][4] and "classify" not in single and "haplotypes" not in single


def test_run_hot_path_samples_is_pinned(gpu_api, single):
    pin.check_samples(gpu_api, single)
