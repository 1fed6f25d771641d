"""ProverSetup(lean=True) sets BJ_SETUP_LEAN for the creation alone: whatever the environment held comes back, also when the
creation raises.  No GPU: the context is a stand-in and the library's entry points are replaced by recorders, so the refusal is the
binding's own path through a failing bj_setup_create."""
import os

import pytest

import era_boojum_amd as E
from era_boojum_amd import binding, synthetic as S


class _Lib:
    """The three entry points the constructor reaches, recording what the environment held when each was called."""

    def __init__(self):
        self.seen = []

    def bj_env_reload(self):
        self.seen.append(("reload", os.environ.get("BJ_SETUP_LEAN")))

    def bj_setup_create(self, *args):
        self.seen.append(("create", os.environ.get("BJ_SETUP_LEAN")))
        return 2                                      # BJ_ERR_NO_DEVICE

    bj_setup_create_sharded = bj_setup_create

    def bj_setup_destroy(self, h):
        pass


class _Ctx:
    def __init__(self):
        self._lib, self._h = _Lib(), None

    def _check(self, rc):
        if rc:
            raise E.BoojumHipError("no usable HIP device")


@pytest.mark.parametrize("before", [None, "0", "1", "yes"])
def test_lean_keyword_restores_the_environment_when_creation_raises(before, monkeypatch):
    if before is None:
        monkeypatch.delenv("BJ_SETUP_LEAN", raising=False)
    else:
        monkeypatch.setenv("BJ_SETUP_LEAN", before)
    c = S.sha_shaped_circuit(8, seed=1, table_bits=2)
    ctx = _Ctx()
    with pytest.raises(E.BoojumHipError, match="no usable HIP device"):
        binding.ProverSetup(ctx, c, 8, 16, 20, lean=True)
    assert os.environ.get("BJ_SETUP_LEAN") == before
    # set and read before the creation, restored and read again after it
    assert ctx._lib.seen == [("reload", "1"), ("create", "1"), ("reload", before)]
    ctx = _Ctx()
    with pytest.raises(E.BoojumHipError):
        binding.ProverSetup(ctx, c, 8, 16, 20)        # lean=False leaves the switch to the environment
    assert ctx._lib.seen == [("create", before)] and os.environ.get("BJ_SETUP_LEAN") == before


def test_lean_and_comm_exclude_each_other():
    c = S.sha_shaped_circuit(8, seed=1, table_bits=2)
    ctx = _Ctx()
    with pytest.raises(E.BoojumHipError, match="single-GPU"):
        binding.ProverSetup(ctx, c, 8, 16, 20, lean=True, comm=object())
    assert ctx._lib.seen == []
