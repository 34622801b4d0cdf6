"""Host side of the one-pass switch (dtc_set_h2i_passes / dtc_get_h2i_passes, h2i.h2i_passes_as, PPO(gemm_passes=...)): declarations,
binding, ABI numbers and the context manager's restore -- no GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "dtc_hip.h")).read()


def test_symbols_are_declared_bound_and_exported():
    import ctypes as C
    from dtc_amd import _ffi
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bvoid\s+dtc_set_h2i_passes\s*\(\s*int\s+passes\s*\)\s*;", code)
    assert re.search(r"\bint\s+dtc_get_h2i_passes\s*\(\s*void\s*\)\s*;", code)
    assert _ffi._SIGS["dtc_set_h2i_passes"] == (None, [C.c_int]) and _ffi._SIGS["dtc_get_h2i_passes"] == (C.c_int, [])
    lib = _ffi.lib()
    assert lib.dtc_get_h2i_passes() == 3
    lib.dtc_set_h2i_passes(2)                                    # refused: says so, changes nothing
    assert lib.dtc_get_h2i_passes() == 3 and b"dtc_set_h2i_passes(2)" in lib.dtc_last_error()
    lib.dtc_set_h2i_passes(1)
    assert lib.dtc_get_h2i_passes() == 1
    lib.dtc_set_h2i_passes(3)
    assert lib.dtc_get_h2i_passes() == 3


def test_abi_numbers_agree():
    from dtc_amd import _ffi
    n = int(re.search(r"#define DTC_ABI_VERSION (\d+)", _header()).group(1))
    assert n == _ffi.ABI_VERSION == _ffi.lib().dtc_version() and n >= 18


class _StubLib:
    def __init__(self):
        self.passes, self.calls = 3, []

    def dtc_set_h2i_passes(self, n):
        self.calls.append(n)
        if n in (1, 3):
            self.passes = n

    def dtc_get_h2i_passes(self):
        return self.passes


def test_context_manager_restores_on_exception(monkeypatch):
    from dtc_amd import h2i
    stub = _StubLib()
    monkeypatch.setattr(h2i, "lib", lambda: stub)
    assert h2i.h2i_passes() == 3
    with h2i.h2i_passes_as(1):
        assert h2i.h2i_passes() == 1
        with h2i.h2i_passes_as(3):                               # nested: each level restores what it found
            assert h2i.h2i_passes() == 3
        assert h2i.h2i_passes() == 1
    assert h2i.h2i_passes() == 3
    with pytest.raises(KeyError):
        with h2i.h2i_passes_as(1):
            assert stub.passes == 1
            raise KeyError("inside")
    assert stub.passes == 3 and stub.calls[-2:] == [1, 3]
    with pytest.raises(ValueError):                              # a bad value: refused before anything is set
        with h2i.h2i_passes_as(2):
            pass
    assert stub.passes == 3 and 2 not in stub.calls
    stub.passes = 1                                              # entered at one pass: leaves at one pass
    with h2i.h2i_passes_as(3):
        assert stub.passes == 3
    assert stub.passes == 1


def test_ppo_keyword_is_keyword_only_and_validated():
    import inspect
    from dtc_amd.algorithms import PPO, RecurrentDecoderPPO, RecurrentPPO
    from dtc_amd.modules import ActorCriticDecoder
    sig = inspect.signature(PPO.__init__)
    assert sig.parameters["gemm_passes"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["gemm_passes"].default == 3
    positional = [n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert positional == ["self", "actor_critic", "num_learning_epochs", "num_mini_batches", "clip_param", "gamma", "lam", "value_loss_coef",
                          "entropy_coef", "learning_rate", "max_grad_norm", "use_clipped_value_loss", "schedule", "desired_kl", "device"]
    assert "gemm_passes" not in inspect.signature(RecurrentPPO.__init__).parameters
    ac = ActorCriticDecoder(53, 1389, 12)
    alg = PPO(ac, device="cpu", gemm_passes=1)
    assert alg.arithmetic == "f16 (block-scaled hi plane, f32 accumulate)"
    assert PPO(ac, device="cpu").arithmetic == "f32 (emulated: f16x2 split per operand, f32 accumulate)"
    with pytest.raises(ValueError):
        PPO(ac, device="cpu", gemm_passes=2)
    assert isinstance(PPO.arithmetic, property) and PPO.arithmetic.fset is None
    # the recurrent decoder trainer shares PPO's constructor but runs its own update: it refuses the keyword instead of ignoring it
    with pytest.raises(TypeError, match="gemm_passes"):
        RecurrentDecoderPPO.__new__(RecurrentDecoderPPO).__init__(ac, device="cpu", gemm_passes=1)
