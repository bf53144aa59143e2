"""Freeze the REAL reference's bf16 ``lm.model`` output on the tiny LLaMA fixture -- TEST INFRASTRUCTURE ONLY.

Run in the build container:  python -m oracle.make_golden_ref_bf16
The reference is built exactly as ``tests/test_oracle_golden.py::test_live_reference_bf16_matches_oracle_bf16`` builds it (the
weights and inputs of ``tests/golden/llama_tiny.npz``, cast to bf16) and its last hidden state is stored as float32 in
``tests/golden/llama_tiny_ref_bf16.npz``, so the test pins the oracle's bf16 rounding points on machines without the reference."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_import  # noqa: E402
from oracle.make_golden import OUT  # noqa: E402
from tests import tiny  # noqa: E402


def reference_bf16_hidden(z):
    """Last hidden state of the reference's ``lm.model`` in bf16 on the inputs and weights of the llama_tiny fixture ``z``."""
    v, l, vocab, W = tiny.weights_from(z)
    d = ref_import.tiny_llama_dir(l.hidden_size, l.intermediate_size, l.num_attention_heads, l.num_hidden_layers)
    vk = dict(image_size=v.image_size, patch_size=v.patch_size, width=v.width, layers=v.layers,
              head_width=v.head_width, mlp_ratio=v.mlp_ratio, n_query=v.n_query, v_query=v.v_query)
    m = ref_import.build_reference(vk, d, True, W).to(torch.bfloat16)
    embeds, mask = torch.from_numpy(z["embeds"]).to(torch.bfloat16), torch.from_numpy(z["mask"])
    with torch.no_grad():
        return m.decoder.lm.model(inputs_embeds=embeds, attention_mask=mask, output_hidden_states=True,
                                  return_dict=True).hidden_states[-1]


def main():
    z = tiny.load(OUT, "llama_tiny.npz")
    h = reference_bf16_hidden(z)
    np.savez(os.path.join(OUT, "llama_tiny_ref_bf16.npz"), hidden_bf16=h.float().numpy(), mask=z["mask"])
    print("wrote", os.path.join(OUT, "llama_tiny_ref_bf16.npz"), tuple(h.shape))


if __name__ == "__main__":
    main()
