"""CPU: host side of the fused Adam / AdamW step (fabind_amd/optim.py): the chunk / row table builder, the ctypes mirror of its row
struct, and the refusal of host parameters."""
import ctypes

import numpy as np
import pytest
import torch

C = 4096
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, C - 1, C, C + 1, 2 * C + 3, 7 * 13, 64 * 65]      # the size list of tests/test_gpu_optim.py


def _static(numels, groups=None):
    from fabind_amd import optim
    rows = np.zeros(len(numels), dtype=optim._ROW)
    rows["p"] = 0x1000 + 0x100000 * np.arange(len(numels))
    rows["m"] = 0x2000 + 0x100000 * np.arange(len(numels))
    rows["v"] = 0x3000 + 0x100000 * np.arange(len(numels))
    rows["numel"] = numels
    rows["step_idx"] = np.arange(len(numels))
    return rows, np.asarray(groups if groups is not None else [0] * len(numels), dtype=np.int64)


def test_chunk_size_is_the_kernels():
    from fabind_amd import _lib, optim
    assert optim.CHUNK == C == _lib.load().fabind_adam_chunk()


def test_chunk_prefix_and_binary_search_invariant():
    from fabind_amd import optim
    pre = optim.chunk_prefix(SIZES)
    want = [1] * 10 + [2, 3, 1, 2]                                  # ceil(numel / 4096)
    assert np.diff(pre).tolist() == want and pre[0] == 0 and pre[-1] == sum(want)
    chunk0 = pre[:-1]
    covered = np.zeros(len(SIZES), dtype=np.int64)
    for c in range(int(pre[-1])):
        r = optim.find_row(chunk0, c)
        assert chunk0[r] <= c < pre[r + 1]                          # the row found owns the chunk
        n = min(C, SIZES[r] - (c - int(chunk0[r])) * C)
        assert 1 <= n <= C                                          # no empty chunk, no chunk past the tensor's end
        covered[r] += n
    assert covered.tolist() == SIZES                                # every element is in exactly one chunk
    assert optim.find_row(np.array([0]), 0) == 0                    # a single row


def test_table_drops_empty_tensors_and_missing_gradients():
    from fabind_amd import optim
    numels = [5, 0, C + 1, 7, 3]
    static = _static(numels, groups=[0, 0, 1, 1, 0])
    g = np.array([0x9000, 0x9100, 0x9200, 0, 0x9401], dtype=np.uint64)       # row 3 has no gradient, row 1 no elements
    hyper = np.array([[1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0], [3e-4, 0.8, 0.99, 1e-6, 0.0, 0.0]])
    t, n_chunks = optim.build_table(static, g, hyper)
    assert t["step_idx"].tolist() == [0, 2, 4]                      # the step counters keep the parameter's index
    assert t["numel"].tolist() == [5, C + 1, 3] and t["chunk0"].tolist() == [0, 1, 3] and n_chunks == 4
    assert t["g"].tolist() == [0x9000, 0x9200, 0x9401] and t["p"].tolist() == static[0]["p"][[0, 2, 4]].tolist()
    assert t["lr"].tolist() == [1e-3, 3e-4, 1e-3] and t["beta2"].tolist() == [0.999, 0.99, 0.999]
    assert t["weight_decay"].tolist() == [0.01, 0.0, 0.01] and t["decoupled"].tolist() == [1, 0, 1]
    assert static[0]["g"].tolist() == [0] * 5                       # the cached static part is not written
    t, n_chunks = optim.build_table(static, np.zeros(5, dtype=np.uint64), hyper)
    assert len(t) == 0 and n_chunks == 0


def test_row_struct_mirrors_agree():
    from fabind_amd import _lib, optim
    lib = _lib.load()
    assert lib.fabind_sizeof_args(5) == ctypes.sizeof(_lib.AdamRow) == optim._ROW.itemsize == 96
    assert [n for n, _ in _lib.AdamRow._fields_] == list(optim._ROW.names)
    assert [getattr(_lib.AdamRow, n).offset for n in optim._ROW.names] == [optim._ROW.fields[n][1] for n in optim._ROW.names]
    assert lib.fabind_abi_version() == 19                           # additive: the version did not move


def test_host_parameters_are_refused():
    from fabind_amd.optim import FusedAdam
    with pytest.raises(RuntimeError, match="HIP device"):
        FusedAdam([torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(NotImplementedError):
        FusedAdam([torch.nn.Parameter(torch.zeros(4))], amsgrad=True)
    with pytest.raises(NotImplementedError):
        FusedAdam([torch.nn.Parameter(torch.zeros(4))], maximize=True)
