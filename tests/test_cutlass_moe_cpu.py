"""CPU: cutlass_fused_moe has the reference's signature, lives in flashinfer.fused_moe_16bit, and refuses by name, before any
launch, what its unquantised f16 / bf16 mode does not provide."""
import inspect

import pytest
import torch

REFERENCE_PARAMETERS = [  # flashinfer/fused_moe/core.py:758-786
    "input", "token_selected_experts", "token_final_scales", "fc1_expert_weights", "fc2_expert_weights", "output_dtype",
    "quant_scales", "fc1_expert_biases", "fc2_expert_biases", "input_sf", "swiglu_alpha", "swiglu_beta", "swiglu_limit",
    "tp_size", "tp_rank", "ep_size", "ep_rank", "cluster_size", "cluster_rank", "output", "enable_alltoall",
    "use_deepseek_fp8_block_scale", "use_w4_group_scaling", "use_mxfp8_act_scaling", "min_latency_mode",
    "tune_max_num_tokens", "enable_pdl"]


def _args(T=3, E=4, top_k=2, H=128, I=64, dtype=torch.bfloat16, **over):
    a = dict(input=torch.zeros(T, H, dtype=dtype), token_selected_experts=torch.zeros(T, top_k, dtype=torch.int32),
             token_final_scales=torch.zeros(T, top_k), fc1_expert_weights=torch.zeros(E, 2 * I, H, dtype=dtype),
             fc2_expert_weights=torch.zeros(E, H, I, dtype=dtype), output_dtype=dtype, quant_scales=None)
    a.update(over)
    return a


REFUSED = {
    "fp8_input": dict(input=torch.zeros(3, 128).to(torch.float8_e4m3fn)),
    "f32_input": dict(input=torch.zeros(3, 128)),
    "nvfp4_weights": dict(fc1_expert_weights=torch.zeros(4, 128, 64, dtype=torch.uint8)),
    "quant_scales": dict(quant_scales=[torch.ones(1)]),
    "input_sf": dict(input_sf=torch.ones(1)),
    "fc1_expert_biases": dict(fc1_expert_biases=torch.zeros(4, 128)),
    "fc2_expert_biases": dict(fc2_expert_biases=torch.zeros(4, 128)),
    "enable_alltoall": dict(enable_alltoall=True),
    "use_deepseek_fp8_block_scale": dict(use_deepseek_fp8_block_scale=True),
    "use_w4_group_scaling": dict(use_w4_group_scaling=True),
    "use_mxfp8_act_scaling": dict(use_mxfp8_act_scaling=True),
    "min_latency_mode": dict(min_latency_mode=True),
}
MALFORMED = {
    "fc2_shape": dict(fc2_expert_weights=torch.zeros(4, 128, 128, dtype=torch.bfloat16)),
    "hidden_not_a_multiple_of_64": dict(input=torch.zeros(3, 96, dtype=torch.bfloat16),
                                        fc1_expert_weights=torch.zeros(4, 128, 96, dtype=torch.bfloat16),
                                        fc2_expert_weights=torch.zeros(4, 96, 64, dtype=torch.bfloat16)),
    "output_dtype": dict(output_dtype=torch.float16),
    "f32_ids": dict(token_selected_experts=torch.zeros(3, 2)),
    "bf16_scales": dict(token_final_scales=torch.zeros(3, 2, dtype=torch.bfloat16)),
    "alpha_alone": dict(swiglu_alpha=torch.ones(4)),
    "ep_rank": dict(ep_size=2, ep_rank=2),
}


@pytest.mark.parametrize("name", sorted(REFUSED) + sorted(MALFORMED))
def test_refused_arguments_raise_before_any_launch(name):
    """Every tensor here lives on the CPU: reaching a kernel, or the check that a tensor is on the GPU, would raise
    RuntimeError instead."""
    import flashinfer

    layer = flashinfer.fused_moe_16bit.cutlass_fused_moe
    assert list(inspect.signature(layer).parameters) == REFERENCE_PARAMETERS
    error = NotImplementedError if name in REFUSED else ValueError
    with pytest.raises(error):
        layer(**_args(**{**REFUSED, **MALFORMED}[name]))
    with pytest.raises(RuntimeError, match="GPU"):  # the same call without the offending argument gets past validation
        layer(**_args())
