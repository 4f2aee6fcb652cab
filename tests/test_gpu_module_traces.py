"""The module layer asks of mio.ops exactly what it asked when tests/golden/module_traces.json was recorded (tests/_module_trace.py):
per case the same calls in the same order with the same flags, shapes, strides, dtypes and kernel routes, a second run without
weight preparation, and the same output bytes.  One test function per module class, one case per parameter."""
import pytest

import _module_trace as mt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return mt.load_golden()


def _check(name, golden):
    got, want = mt.run_case(mt.case(name)), golden[name]
    for i, (g, w) in enumerate(zip(got["trace"], want["trace"])):
        assert g == w, f"{name}: call {i} differs from the record"
    assert len(got["trace"]) == len(want["trace"]), f"{name}: {len(got['trace'])} calls, the record has {len(want['trace'])}"
    assert want["digest"] is not None and got["digest"] == want["digest"], f"{name}: output bytes differ from the record"


def test_every_case_is_recorded(golden):
    assert sorted(golden) == sorted(c.name for c in mt.CASES)
    assert {c.cls for c in mt.CASES} == set(mt.CLASSES)


@pytest.mark.parametrize("name", mt.case_names("FlashSelfAttention"))
def test_flash_self_attention(name, golden):
    _check(name, golden)


@pytest.mark.parametrize("name", mt.case_names("FlashAttentionLayer"))
def test_flash_attention_layer(name, golden):
    _check(name, golden)


@pytest.mark.parametrize("name", mt.case_names("RingAttention"))
def test_ring_attention(name, golden):
    _check(name, golden)


@pytest.mark.parametrize("name", mt.case_names("RingCrossAttention"))
def test_ring_cross_attention(name, golden):
    _check(name, golden)


@pytest.mark.parametrize("name", mt.case_names("FusedTransformerMLP"))
def test_fused_transformer_mlp(name, golden):
    _check(name, golden)


@pytest.mark.parametrize("name", mt.case_names("synthetic"))
def test_synthetic_blocks(name, golden):
    _check(name, golden)
