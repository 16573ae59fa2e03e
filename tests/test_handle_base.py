"""The one handle base (fleet_amd._capi.Handle): destroy is called once, only while every owner
up the chain is open, and each real class declares the chain its own ``close`` spelled out by
hand before the base existed. No library, no GPU: the destroy function is a fake that records."""
import gc
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fleet_amd._capi import Handle  # noqa: E402


class _Lib:
    def __init__(self, fail=False):
        self.destroyed, self.fail = [], fail

    def fake_destroy(self, h):
        self.destroyed.append(h)
        if self.fail:
            raise RuntimeError("destroy failed")


class _Owner:
    def __init__(self, h=1, **attrs):
        self._h = h
        self.__dict__.update(attrs)


class _Leaf(Handle):
    _destroy, _owners, _closed = "fake_destroy", ("ledger", "pool", "pool.codec"), "the leaf or an owner is closed"

    def __init__(self, lib, ledger, pool, h=7, fail_early=False):
        self._L, self.ledger, self.pool = lib, ledger, pool
        if fail_early:
            raise ValueError("before there is a handle")
        self._h = h


def _chain():
    codec = _Owner(h=3)
    pool = _Owner(h=2, codec=codec)
    return _Lib(), _Owner(h=1), pool, codec


def test_destroy_once_on_close_and_never_again():
    lib, ledger, pool, _ = _chain()
    leaf = _Leaf(lib, ledger, pool)
    leaf.close()
    assert lib.destroyed == [7] and leaf._h is None
    leaf.close()
    leaf.__del__()
    del leaf
    gc.collect()
    assert lib.destroyed == [7]


def test_context_manager_closes():
    lib, ledger, pool, _ = _chain()
    with _Leaf(lib, ledger, pool) as leaf:
        assert leaf._live() == 7
    assert lib.destroyed == [7] and leaf._h is None


@pytest.mark.parametrize("closed", ["ledger", "pool", "codec"])
def test_no_destroy_once_any_owner_is_closed(closed):
    lib, ledger, pool, codec = _chain()
    leaf = _Leaf(lib, ledger, pool)
    {"ledger": ledger, "pool": pool, "codec": codec}[closed]._h = None
    with pytest.raises(ValueError, match="the leaf or an owner is closed"):
        leaf._live()
    leaf.close()
    assert lib.destroyed == [] and leaf._h is None


def test_close_of_a_half_constructed_object_is_silent():
    lib, ledger, pool, _ = _chain()
    leaf = _Leaf.__new__(_Leaf)
    with pytest.raises(ValueError, match="before there is a handle"):
        leaf.__init__(lib, ledger, pool, fail_early=True)
    assert not hasattr(leaf, "_h")
    leaf.close()
    leaf.__del__()
    assert lib.destroyed == []
    bare = _Leaf.__new__(_Leaf)  # __init__ raised before any attribute was set
    bare.close()
    bare.__del__()


def test_del_swallows_what_destroy_raises():
    lib, ledger, pool, _ = _chain()
    lib.fail = True
    leaf = _Leaf(lib, ledger, pool)
    leaf.__del__()
    assert lib.destroyed == [7]
    with pytest.raises(RuntimeError):
        _Leaf(lib, ledger, pool, h=8).close()


def test_live_returns_the_handle_while_everything_is_open():
    lib, ledger, pool, _ = _chain()
    leaf = _Leaf(lib, ledger, pool)
    assert leaf._live() == 7
    leaf.close()
    with pytest.raises(ValueError, match="the leaf or an owner is closed"):
        leaf._live()


# the owners in each class's destroy guard, copied by hand from the close() bodies the base replaced
GUARDS = {
    "Codec": ("fleet_destroy", ()),
    "Accumulator": ("fleet_acc_destroy", ("codec",)),
    "Pool": ("fleet_pool_destroy", ("codec",)),
    "Gate": ("fleet_gate_destroy", ("pool", "pool.codec")),
    "Ledger": ("fleet_kledger_destroy", ("pool", "pool.codec")),
    "KardamFilter": ("fleet_kfilter_destroy", ("ledger", "pool", "pool.codec")),
    "ModelLedger": ("fleet_mledger_destroy", ("codec",)),
    "Model": ("fleet_model_destroy", ()),
    "ResidentModel": ("fleet_rmodel_destroy", ()),
}
MESSAGES = {"Gate": "the gate or its pool is closed", "Ledger": "the ledger or its pool is closed",
            "KardamFilter": "the filter is closed", "ModelLedger": "the model ledger or its codec is closed"}


def test_each_class_declares_the_guard_it_had():
    import fleet_amd
    from fleet_amd._capi import SIGNATURES
    handles = {n for n, c in vars(fleet_amd).items() if isinstance(c, type) and issubclass(c, Handle)}
    assert handles == set(GUARDS)
    for name, (destroy, owners) in GUARDS.items():
        cls = getattr(fleet_amd, name)
        assert (cls._destroy, cls._owners) == (destroy, owners), name
        assert destroy in SIGNATURES
        assert "close" not in vars(cls) and "__del__" not in vars(cls), name
    for name, text in MESSAGES.items():
        assert getattr(fleet_amd, name)._closed == text


def test_the_filter_asks_its_ledger():
    """KardamFilter._live: its own message when it is closed, the ledger's when the ledger is."""
    from fleet_amd import KardamFilter, Ledger
    codec = _Owner(h=3)
    pool = _Owner(h=2, codec=codec)
    ledger = Ledger.__new__(Ledger)
    ledger._h, ledger.pool = 5, pool
    f = KardamFilter.__new__(KardamFilter)
    f._h, f.ledger, f.pool = 9, ledger, pool
    assert f._live() == 9
    pool._h = None
    with pytest.raises(ValueError, match="the ledger or its pool is closed"):
        f._live()
    f._h = None
    with pytest.raises(ValueError, match="the filter is closed"):
        f._live()
    ledger._h = None  # nothing to destroy: no library is touched when the two are collected
