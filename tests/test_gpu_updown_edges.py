"""updown_block on the device at every launch class, chunk, batch and failure edge: the cases of
tests/updown_cases.py.  For every case L.x after the device call is byte-equal to the reference loop of
csparse_oracle.cs_updown on the same inputs (run on the CPU, once per case) with the same count applied; updown_info() reports
the classes, chunks, groups and union columns of the CPU model of the schedule (updown_block_oracle.schedule) and whether the
replay ran; and the device's own loop of cs_updown is byte-equal too, which puts k_updown on the same edges.  The failing
cases run again all or nothing (L.x untouched, the same count), and the call after a refused or failed one is right.
Everything is byte equality: no tolerances."""
import numpy as np
import pytest

import updown_block_oracle as UB
import updown_cases as UC
from test_gpu_parity import cs  # noqa: F401
from test_gpu_updown_block import _dev_cs, _loop, _xb

pytestmark = pytest.mark.gpu

ALL_OR_NOTHING, CHECK_PATTERN = 1, 2


def _L(cs, c):
    return _dev_cs(cs, c.n, c.p, c.i, c.x)


def _C(cs, c, cols=None):
    return UC.columns(cs, c.n, c.cols if cols is None else cols)


def _parent(c):
    return UB.tree_of(c.oracle_L())


def _model(c, cols=None):
    C = c.oracle_C() if cols is None else UC.columns(UC.O, c.n, cols)
    return UB.schedule_facts(UB.schedule(c.oracle_L(), C))


def _call(cs, L, sigma, C, flags, parent=None):
    """csx_updown_block with flags, through the wrapper's own bookkeeping"""
    return cs._updown_block_call(L, cs._updown_sigma(sigma, C.n), C, parent, flags)


def _route(info):
    return {key: info[key] for key in ("chunks", "groups", "union_columns", "classes")}


@pytest.mark.parametrize("name", UC.NAMES)
def test_block_is_the_reference_loop(cs, name):
    c = UC.get(name)
    L = _L(cs, c)
    assert cs.updown_block(L, c.sigma, _C(cs, c)) == c.applied
    info = cs.updown_info()
    assert _xb(L) == c.ref_x
    assert _route(info) == _model(c) and info["replayed"] == int(c.fails)
    assert info["columns"] == c.k and info["applied"] == c.applied
    for key in ("classes", "union_columns", "chunks"):            # the model's word is the case's stated edge
        assert info[key] == c.expect.get(key, info[key])
    # the device's loop of rank-1 calls: k_updown on the same edges
    La = _L(cs, c)
    assert _loop(cs, La, c.sigma, c.cols, _parent(c)) == c.applied
    assert _xb(La) == c.ref_x


@pytest.mark.parametrize("name", UC.FAILING)
@pytest.mark.parametrize("flags", [ALL_OR_NOTHING, ALL_OR_NOTHING | CHECK_PATTERN])
def test_all_or_nothing_leaves_L_and_the_next_call_is_right(cs, name, flags):
    c = UC.get(name)
    L = _L(cs, c)
    C = _C(cs, c)
    assert _call(cs, L, c.sigma, C, flags) == c.applied
    info = cs.updown_info()
    assert _xb(L) == c.x.tobytes()
    assert _route(info) == _model(c) and info["replayed"] == 0  # the first pass ran, the replay did not
    assert _call(cs, L, c.sigma, C, 0) == c.applied               # the same L again: the loop's partial state
    assert _xb(L) == c.ref_x and cs.updown_info()["replayed"] == 1


@pytest.mark.parametrize("name", ["fail_first_upstream", "fail_upstream", "zero_beta2_only", "dup_rows", "n1"])
def test_list_backed_L_follows_the_device(cs, name):
    """L.x held by the caller as a list: the loop's partial state arrives in it also when nothing was applied in full, and
    an all-or-nothing failure leaves the list as it was"""
    c = UC.get(name)
    L = UC.csc(cs, c.n, c.n, c.p, c.i, c.x)
    xlist = L.x
    if c.fails:
        assert _call(cs, L, c.sigma, _C(cs, c), ALL_OR_NOTHING) == c.applied
        assert L.x is xlist and np.asarray(L.x).tobytes() == c.x.tobytes()
    assert cs.updown_block(L, c.sigma, _C(cs, c)) == c.applied
    assert L.x is xlist and np.asarray(L.x).tobytes() == c.ref_x


def test_rows_off_the_path(cs):
    """ignored as the loop ignores them; with the pattern check they refuse the call: -1, L untouched, nothing scheduled, and
    the next call on the same L is right"""
    c = UC.get("off_path")
    L = _L(cs, c)
    C = _C(cs, c)
    for flags in (CHECK_PATTERN, CHECK_PATTERN | ALL_OR_NOTHING):
        assert _call(cs, L, c.sigma, C, flags) == -1
        assert _xb(L) == c.x.tobytes()
        info = cs.updown_info()
        assert info["chunks"] == 0 and info["classes"] == [0, 0, 0, 0] and info["replayed"] == 0
    assert _call(cs, L, c.sigma, C, 0) == c.applied
    assert _xb(L) == c.ref_x
    on = _L(cs, c)                                                # without the two rows off the path: the check passes
    cols = [(c.cols[0][0][:-2], c.cols[0][1][:-2])] + c.cols[1:]
    assert _call(cs, on, c.sigma, _C(cs, c, cols), CHECK_PATTERN) == c.applied
    assert _xb(on) == c.ref_x


@pytest.mark.parametrize("name", ["chunks_uneven", "off_path", "isolated_root", "n1", "fail_chunk0_skips_chunk1"])
def test_parent_given_and_wrong(cs, name):
    c = UC.get(name)
    par = _parent(c)
    L = _L(cs, c)
    wrong = list(par)
    wrong[0] = c.n - 1 if par[0] != c.n - 1 else -1
    with pytest.raises(ValueError):
        cs.updown_block(L, c.sigma, _C(cs, c), wrong)
    assert _xb(L) == c.x.tobytes()
    assert cs.updown_block(L, c.sigma, _C(cs, c), par) == c.applied   # the refused L again, with the right tree
    assert _xb(L) == c.ref_x
    assert _route(cs.updown_info()) == _model(c)


@pytest.mark.parametrize("name,cut", [("staggered", 70), ("sparse_masks", 64), ("chunks_uneven", 100), ("four_classes", 130)])
def test_two_calls_back_to_back(cs, name, cut):
    """the terms in two calls on one L: other unions, other places of the same columns in them, the same bytes in the end"""
    c = UC.get(name)
    L = _L(cs, c)
    assert cs.updown_block(L, c.sigma[:cut], _C(cs, c, c.cols[:cut])) == cut
    assert _route(cs.updown_info()) == _model(c, c.cols[:cut])
    assert cs.updown_block(L, c.sigma[cut:], _C(cs, c, c.cols[cut:])) == c.k - cut
    assert _route(cs.updown_info()) == _model(c, c.cols[cut:])
    assert _xb(L) == c.ref_x
