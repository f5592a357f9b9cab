"""What a CPU test and its GPU twin share that is no reference and no case: a free port for the two data-parallel
tests, and the reference's ragged-read fixture for tests/test_ragged_reads.py and tests/test_gpu_reads.py."""
import os
import socket

import numpy as np
import pytest
import torch

RAGGED_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ragged_00.npz")


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.fixture(scope="module")
def gold():
    """tests/golden/ragged_00.npz as a dict; a test module imports this name to use it"""
    z = np.load(RAGGED_FIXTURE, allow_pickle=False)
    return {k: z[k] for k in z.files}


def ragged_table(gold):
    return torch.from_numpy(gold["table.means"]), torch.from_numpy(gold["table.stdvs"])
