"""The shared primitives of the point-cloud back end on their own -- the one-workgroup exclusive scan of
csrc/device_prims.h (sdpk_block_scan) and the stable radix sort of csrc/radix_sort.hip (sdpk_radix_sort) -- against
numpy, every element exact.  Sizes are the smallest that reach each path, so nothing here needs a million points.

Scan: 4096 counts per iteration (SCAN, read from the header).  n = 1, 63, 64, 65 (one lane either side of a wave),
1023, SCAN - 1, SCAN, SCAN + 1 (the second iteration and its carry), 2 * SCAN + 1, 3 * SCAN + 5; values random in
[0, 256], all zero, all 256 (the largest count a chunk can hold).  Expected: np.cumsum shifted by one and the total;
the elements past n of a longer buffer keep their sentinel.

Sort: 1024 keys per tile (TILE); the digit scan runs over 256 * tiles counts, so it needs a second iteration from 17
tiles on.  n = 1, 2, 255, 256, 257, TILE - 1, TILE, TILE + 1, 4 * TILE + 1, 17 * TILE + 1; key widths 0, 1, 8, 9, 40, 64
bits.  Keys: random below 2^bits; all equal (every pass skipped, the result stays in buffer 0); eight distinct keys with
many repeats; and, at 40 bits, keys that differ only in their top byte (passes 0-3 are skipped by the same-digit rule
and the ping/pong index must follow).  With values (arange(n), 5 passes up to 40 bits like the voxel sort, else 8) the
expected order is np.argsort(keys, kind="stable"), which also proves stability; without values (8 passes, like the label
sort) the sorted keys.  Which buffer holds the result is read from the sort state, as the consumers do, and the whole
state -- the buffer every pass read, which passes moved anything -- is compared with the one numpy derives from the
digits.  Rows past n keep their sentinels in both buffers.  A set "do nothing" flag leaves buffers, counts and state alone.
"""
import os
import re

import numpy as np
import pytest
import torch

import kernel_lib as KL
from conftest import PKG_DIR

pytestmark = pytest.mark.gpu


def _constants():
    src = "".join(open(os.path.join(PKG_DIR, "csrc", f)).read() for f in ("device_prims.h", "radix_sort.h"))
    get = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    hdr = open(os.path.join(os.path.dirname(PKG_DIR), "include", "sdp_kernels.h")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, hdr).group(1))
    return (get("SCAN_THREADS") * get("SCAN_PER_THREAD"), get("RADIX_TILE"), get("RADIX_MAX_PASSES"),
            define("SDPK_RADIX_STATE_INTS"), define("SDPK_RADIX_STATE_RESULT"))


SCAN, TILE, MAX_PASSES, STATE_INTS, STATE_RESULT = _constants()
assert (SCAN, TILE, MAX_PASSES) == (4096, 1024, 8) and STATE_INTS == 2 * MAX_PASSES + 2 and STATE_RESULT == STATE_INTS - 1
SCAN_N = [1, 63, 64, 65, 1023, SCAN - 1, SCAN, SCAN + 1, 2 * SCAN + 1, 3 * SCAN + 5]
SORT_N = [1, 2, 255, 256, 257, TILE - 1, TILE, TILE + 1, 4 * TILE + 1, 17 * TILE + 1]
assert 256 * -(-SORT_N[-1] // TILE) > SCAN >= 256 * -(-SORT_N[-2] // TILE)      # only the last needs a second iteration
BITS = [0, 1, 8, 9, 40, 64]
PAD = 5                       # rows past n in every buffer
KEY_FILL, VAL_FILL, CNT_FILL = -7, -9, -11


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("values", ["random", "zero", "full"])
@pytest.mark.parametrize("n", SCAN_N)
def test_block_scan(n, values):
    rng = np.random.default_rng([n, len(values)])
    c = {"random": rng.integers(0, 257, n), "zero": np.zeros(n), "full": np.full(n, 256)}[values].astype(np.int32)
    data = dev(np.concatenate((c, np.full(PAD, CNT_FILL, np.int32))))
    total = torch.full((1,), CNT_FILL, dtype=torch.int32, device="cuda")
    KL.check(KL.lib().sdpk_block_scan(KL.ptr(data), n, KL.ptr(total), KL.stream()), "block_scan")
    got = data.cpu().numpy()
    inc = np.cumsum(c, dtype=np.int64)
    assert np.array_equal(got[:n], np.concatenate(([0], inc[:-1])))
    assert int(total.item()) == int(inc[-1])
    assert (got[n:] == CNT_FILL).all()


def make_keys(pattern, n, bits, rng):
    mask = np.uint64((1 << bits) - 1)
    rand = lambda size: rng.integers(0, 1 << 64, size, dtype=np.uint64) & mask
    if pattern == "random":
        return rand(n)
    if pattern == "equal":
        return np.full(n, np.uint64(0xA5A5A5A5A5A5A5A5) & mask)
    if pattern == "eight":
        return rand(8)[rng.integers(0, 8, n)]
    assert pattern == "top" and bits == 40
    return np.uint64(0x5A3C9601) | (rng.integers(0, 256, n).astype(np.uint64) << np.uint64(32))


def expected_state(keys, bits, passes):
    """RadixState as numpy derives it: src[9] (the buffer pass p reads), active[8], result."""
    src, active = np.zeros(MAX_PASSES + 1, np.int32), np.zeros(MAX_PASSES, np.int32)
    for p in range(passes):
        digit = (keys >> np.uint64(8 * p)) & np.uint64(255)
        active[p] = int(8 * p < bits and len(np.unique(digit)) > 1)
        src[p + 1] = src[p] ^ active[p]
    return np.concatenate((src, active, [src[passes]])).astype(np.int32)


def run_sort(keys, bits, passes, with_values, skip=0, state_fill=0):
    n = len(keys)
    cap = n + PAD
    tail = np.full(PAD, KEY_FILL, np.int64)
    key = [dev(np.concatenate((keys.view(np.int64), tail))), torch.full((cap,), KEY_FILL, dtype=torch.int64, device="cuda")]
    val = [None, None]
    if with_values:
        val = [dev(np.concatenate((np.arange(n, dtype=np.int32), np.full(PAD, VAL_FILL, np.int32)))),
               torch.full((cap,), VAL_FILL, dtype=torch.int32, device="cuda")]
    cnt = torch.full((256 * -(-cap // TILE),), CNT_FILL, dtype=torch.int32, device="cuda")
    params = dev(np.array([n, bits, skip], np.int32))
    state = torch.full((STATE_INTS,), state_fill, dtype=torch.int32, device="cuda")
    KL.check(KL.lib().sdpk_radix_sort(KL.ptr(key[0]), KL.ptr(key[1]), KL.ptr(val[0]), KL.ptr(val[1]), KL.ptr(cnt), cap,
                                      KL.ptr(params), KL.ptr(state), passes, KL.stream()), "radix_sort")
    host = lambda t: None if t is None else t.cpu().numpy()
    return [host(k) for k in key], [host(v) for v in val], host(cnt), host(state)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n", SORT_N)
def test_radix_sort(n, bits):
    rng = np.random.default_rng([n, bits])
    for pattern in ["random", "equal", "eight"] + (["top"] if bits == 40 else []):
        keys = make_keys(pattern, n, bits, rng)
        order = np.argsort(keys, kind="stable")
        for with_values in (True, False):
            passes = 5 if with_values and bits <= 40 else MAX_PASSES
            what = (pattern, with_values)
            key, val, _, state = run_sort(keys, bits, passes, with_values)
            assert np.array_equal(state, expected_state(keys, bits, passes)), what
            r = int(state[STATE_RESULT])
            if pattern == "equal":
                assert r == 0 and not state[MAX_PASSES + 1:STATE_RESULT].any(), what
            if pattern == "top" and len(np.unique(keys)) > 1:
                assert r == 1 and list(state[MAX_PASSES + 1:STATE_RESULT]) == [0, 0, 0, 0, 1, 0, 0, 0], what
            assert np.array_equal(key[r][:n].view(np.uint64), keys[order]), what
            assert (key[0][n:] == KEY_FILL).all() and (key[1][n:] == KEY_FILL).all(), what
            if with_values:
                assert np.array_equal(val[r][:n], order), what
                assert (val[0][n:] == VAL_FILL).all() and (val[1][n:] == VAL_FILL).all(), what


@pytest.mark.parametrize("with_values", [True, False])
def test_radix_sort_do_nothing_flag(with_values):
    n = 4 * TILE + 1
    keys = make_keys("random", n, 40, np.random.default_rng(7))
    key, val, cnt, state = run_sort(keys, 40, MAX_PASSES, with_values, skip=1, state_fill=-5)
    assert np.array_equal(key[0][:n].view(np.uint64), keys) and (key[0][n:] == KEY_FILL).all() and (key[1] == KEY_FILL).all()
    if with_values:
        assert np.array_equal(val[0][:n], np.arange(n)) and (val[0][n:] == VAL_FILL).all() and (val[1] == VAL_FILL).all()
    assert (cnt == CNT_FILL).all() and (state == -5).all()


def test_rejected_calls_launch_nothing():
    L = KL.lib()
    t = torch.zeros(STATE_INTS, dtype=torch.int32, device="cuda")
    k = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert L.sdpk_block_scan(KL.ptr(t), -1, KL.ptr(t), KL.stream()) != 0
    assert L.sdpk_radix_sort(KL.ptr(k), KL.ptr(k), KL.ptr(t), None, KL.ptr(t), 4, KL.ptr(t), KL.ptr(t), 8, KL.stream()) != 0
    assert L.sdpk_radix_sort(KL.ptr(k), KL.ptr(k), None, None, KL.ptr(t), 4, KL.ptr(t), KL.ptr(t), 9, KL.stream()) != 0
    assert L.sdpk_radix_sort(KL.ptr(k), KL.ptr(k), None, None, KL.ptr(t), 0, KL.ptr(t), KL.ptr(t), 8, KL.stream()) != 0
