"""CPU: the video-QA surface of ABI 22 -- exported symbols, host-side refusals of the bindings, and the evaluation driver's argument check
(none of them touches a GPU)."""
import os
import re

import pytest
import torch

from tests.conftest import ROOT


def test_qa_symbols_are_exported_and_declared():
    from alpro_amd import hip
    hdr = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    lib = hip.load()
    for name in ("alpro_gemm_rows_f32_relu_mask", "alpro_clip_pool"):
        assert name in hip.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, hdr)
        getattr(lib, name)
    assert hip.ABI_VERSION == 22 == lib.alpro_hip_abi_version()
    assert int(re.search(r"ALPRO_ACT_RELU_MASK = (\d+)", hdr).group(1)) == hip.ACT_RELU_MASK
    for mode, code in hip.POOL_MODES.items():
        assert int(re.search(r"ALPRO_POOL_%s = (\d+)" % mode.upper(), hdr).group(1)) == code


def test_qa_bindings_refuse_cpu_tensors():
    from alpro_amd import hip
    x = torch.zeros(6, 64)
    with pytest.raises(RuntimeError, match="device tensors"):
        hip.clip_pool(x, 3, "mean")
    with pytest.raises(RuntimeError, match="device tensors"):
        hip.gemm_rows_relu_mask(x, torch.zeros(16, 64), torch.zeros(6, 16))
    with pytest.raises(RuntimeError, match="device tensors"):
        hip.gemm_rows(x, torch.zeros(1500, 64), act=hip.ACT_RELU)
    with pytest.raises(ValueError, match="mode"):
        hip.clip_pool(x, 3, "median")


def test_inference_qa_rejects_an_unknown_pooling_before_touching_the_device():
    from alpro_amd.qa_eval import inference_qa

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the model was used before the argument check (%s)" % name)

    def batches():
        raise AssertionError("the batches were read before the argument check")
        yield

    with pytest.raises(ValueError, match="pool_method"):
        inference_qa(Untouchable(), batches(), num_clips=4, num_frm=16, score_agg_func="median")


def test_qa_model_has_no_eager_head_left():
    """The answer head runs on the library: no F.relu / F.cross_entropy / torch.cat in AlproForSequenceClassification."""
    import inspect
    from alpro_amd.modeling import alpro_models as am
    src = inspect.getsource(am.AlproForSequenceClassification) + inspect.getsource(am._QAHead)
    for banned in ("F.relu(", "F.cross_entropy(", "torch.cat("):
        assert banned not in src, banned
