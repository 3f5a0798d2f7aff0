"""Shared pytest setup.

* ``gpu`` marker: tests that need a real MI355X (run with ``-m gpu`` on the GPU box).
* ``data_root`` / ``cleaned`` / ``daily`` fixtures: the reference dataset (cleaned_data + raw data/ +
  the shipped generators) from tests/golden/reference, so every test runs from the repository alone.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import hfrep  # noqa: E402  (registers the package)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an AMD MI355X GPU (gfx950) and the native kernel library")
    config.addinivalue_line("markers", "slow: long-running test")


GOLDEN = os.path.join(ROOT, "tests", "golden", "reference")


@pytest.fixture(scope="session")
def data_root(tmp_path_factory):
    """A root with the RAW reference data (data/), cleaned_data/ and the shipped generators (GAN/): the
    files stored under tests/golden/reference in the reference layout, the CSV files (stored xz-packed)
    unpacked under their own names.  Also the session's ``HFREP_DATA_ROOT``, so library calls that look
    the dataset up themselves read the same files."""
    import lzma

    root = tmp_path_factory.mktemp("reference")
    for d, _, files in os.walk(GOLDEN):
        out = root / os.path.relpath(d, GOLDEN)
        out.mkdir(exist_ok=True)
        for f in files:
            src = os.path.join(d, f)
            if f.endswith(".xz"):
                with lzma.open(src) as fh:
                    (out / f[:-3]).write_bytes(fh.read())
            else:
                os.symlink(src, out / f)
    os.environ["HFREP_DATA_ROOT"] = str(root)
    return str(root)


@pytest.fixture(scope="session")
def cleaned(data_root):
    """The cleaned panel (cleaned_data/)."""
    from hfrep.data.io import load_cleaned

    return load_cleaned(data_root)


@pytest.fixture
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from hfrep.ops import _native

    _native.native()  # must load on a GPU box
    return torch.device("cuda")


@pytest.fixture(scope="session")
def daily(data_root):
    """The daily ETF excess-return matrix, built from the raw prices."""
    from hfrep.data.io import load_daily_etf

    return load_daily_etf(data_root)[0]
