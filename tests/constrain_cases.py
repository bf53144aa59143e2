"""Inputs shared by tests/test_constrain_host.py (CPU) and tests/test_gpu_constrain.py: the tries, the node shapes of the kernel
tests, and the tiny random LLaMA that the host loops are compared on against the installed library."""
import torch

from emu_amd.constrain import TokenTrie

EOS, PAD = 2, 32000
# shared prefixes, one sequence a prefix of another, and so few branches that the finite candidates stay below 2N at every step
LIB_SEQS = [[10, 11], [10, 12, 13], [20], [21, 22, 23, 24], [10, 11, 30]]


def random_sequences(n, length, vocab, seed, eos=EOS):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab, (n, length), generator=g)
    return [[int(t) for t in row if int(t) != eos] or [3] for row in ids]


def node_shape_tries(V, nb, eos=EOS):
    """name -> (trie, node index the rows stand at): one case per shape of the node the mask is read from.  Every trie is built from
    sequences, so that each case also passes through ``TokenTrie``'s own numbering."""
    def fan(k):
        ids = [t for t in torch.randperm(V, generator=torch.Generator().manual_seed(V + k)).tolist() if t != eos][:k]
        return TokenTrie([[t] for t in ids], eos, V), 0
    cases = {"fan1": fan(1), "fan2": fan(2), "fan2N-1": fan(2 * nb - 1), "fan2N+3": fan(min(2 * nb + 3, V - 1))}
    edge = sorted({t for t in (0, 1023, 1024, V - 1) if t < V and t != eos})
    cases["chunk_edges"] = (TokenTrie([[t] for t in edge], eos, V), 0)
    cases["exhausted"] = (TokenTrie([[5]], eos, V), -1)
    # every id a child: all V - 1 other ids continue, and EOS itself ends the (second-level) sequence
    deep = TokenTrie([[7, t] for t in range(V) if t != eos] + [[7]], eos, V)
    cases["all"] = (deep, deep.walk([7]))
    return cases


def tiny_llama(seed, vocab=64, hidden=32, heads=4, layers=2, ffn=64):
    """(transformers LlamaForCausalLM with random weights, the same weights under the oracle's names, the product's and the oracle's
    config) -- fp32, on the CPU."""
    from transformers import LlamaConfig, LlamaForCausalLM
    from emu_amd.conf.emu_conf import LlamaCfg
    from oracle import emu2_ref as R
    torch.manual_seed(seed)
    hf = LlamaForCausalLM(LlamaConfig(vocab_size=vocab, hidden_size=hidden, intermediate_size=ffn, num_hidden_layers=layers,
                                      num_attention_heads=heads, num_key_value_heads=heads, max_position_embeddings=128,
                                      rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=False, attention_bias=False,
                                      bos_token_id=1, eos_token_id=EOS, pad_token_id=0)).eval()
    with torch.no_grad():
        hf.lm_head.weight.mul_(8.0)                   # a peaked distribution: margins between candidates well above rounding
    W = {"decoder.lm." + k: v.detach().clone() for k, v in hf.state_dict().items()}
    l = LlamaCfg(hidden_size=hidden, intermediate_size=ffn, num_attention_heads=heads, num_hidden_layers=layers,
                 max_position_embeddings=128)
    r = R.LlamaCfg(hidden=hidden, heads=heads, layers=layers, ffn=ffn, vocab=vocab, rms_eps=1e-6, rope_theta=10000.0, max_pos=128)
    return hf, W, l, r
