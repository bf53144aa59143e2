"""Freeze what the tests need from the reference's ``llama_config`` directory into tests/golden/  -- TEST INFRASTRUCTURE ONLY.

Run in the build container:  python -m oracle.make_golden_llama_config
Stored in ``tests/golden/llama_config_ref.json``: the ids the reference tokenizer assigns to the Emu special tokens, its length
with and without the instruct tokens, the ids of the placeholder prompt ``tests/test_chat_host.py`` encodes, and the tensor names
of the reference's ``pytorch_model.bin.index.json`` (rotary ``inv_freq`` buffers dropped).  Nothing else of the directory."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_import  # noqa: E402
from oracle.make_golden import OUT  # noqa: E402
from emu_amd import constants as K  # noqa: E402
from emu_amd.emu import build_tokenizer  # noqa: E402

PLACEHOLDER_PROMPT = K.DEFAULT_IMG_TOKEN + K.DEFAULT_IMAGE_TOKEN * 4 + K.DEFAULT_IMG_END_TOKEN + "describe"


def main():
    tok = build_tokenizer(ref_import.REF_LLAMA_CFG, instruct=True)
    special = [K.DEFAULT_PAD_TOKEN, K.DEFAULT_IMG_TOKEN, K.DEFAULT_IMG_END_TOKEN, K.DEFAULT_IMAGE_TOKEN, K.DEFAULT_gIMG_TOKEN]
    wm = json.load(open(os.path.join(ref_import.REF_LLAMA_CFG, "pytorch_model.bin.index.json")))["weight_map"]
    out = {"special_token_ids": {t: tok.convert_tokens_to_ids(t) for t in special},
           "len_instruct": len(tok), "len_base": len(build_tokenizer(ref_import.REF_LLAMA_CFG, instruct=False)),
           "placeholder_prompt": PLACEHOLDER_PROMPT, "placeholder_prompt_ids": tok(PLACEHOLDER_PROMPT).input_ids,
           "index_tensor_names": sorted(k for k in wm if not k.endswith("rotary_emb.inv_freq"))}
    json.dump(out, open(os.path.join(OUT, "llama_config_ref.json"), "w"), indent=1)
    print("wrote", os.path.join(OUT, "llama_config_ref.json"))


if __name__ == "__main__":
    main()
