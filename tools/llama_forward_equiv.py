"""Bit-for-bit check of emu_llama_forward and emu_llama_logits between two builds of libemu_hip.so: seeded cases over every
schedule of the forward (per-layer launches for decode / prefill / left-padded batch / beam-shaped steps / fp8, decode tail and
merged o_proj, the MXFP4 modes 1-3 at every row range and after release_bf16, the fp8 modes 3, 5 and 6 at 5, 20 and 65 rows with and
without the head's fp8 copy, the 13-bit packed streams at 1, 5 and 16 rows, the fused decode modes 1-4 on the shard-emulation
engines, the two-lane tensor-parallel prefill over p2p and 1-rank RCCL) and every kernel of the head (whole, with the workspace too
small, vocabulary-sharded).  Per case it writes the sha256 of the residual stream forward returned and of the K and V cache it wrote,
of the logits where the case takes them, plus the path counters (the weight-stream profiler's bytes and launches in the fp4, fp8w
and pack groups), as JSON:

    python tools/llama_forward_equiv.py new.json [main|merge|fp4|fp8w|pack|fused|lanes ...]
    EMU_HIP_TOOLS=1 EMU_HIP_LIB=/path/to/other/libemu_hip.so python tools/llama_forward_equiv.py other.json

Equal files = equal bits in every case (profiles/llama_forward_refactor_equivalence.md, profiles/weight_path_refactor_equivalence.md,
profiles/projection_rule_equivalence.md)."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

BF16 = torch.bfloat16
out_path = sys.argv[1] if len(sys.argv) > 1 else "llama_forward_equiv.json"
only = set(sys.argv[2:])
res = {}
WAVE = dict(hidden_size=1024, intermediate_size=2048, num_attention_heads=8, num_hidden_layers=3)   # o_proj / down_proj in the wave forms


class ShardView:                      # rank 0's 1/tp shard of the model; the comm block sees the 1-rank context
    def __init__(self, ctx, size):
        self.__dict__.update(ctx=ctx, tp_rank=0, tp_size=size)

    def __getattr__(self, k):
        return getattr(self.ctx, k)


def make_engine(cfg, vocab, tp=1, comm=None):
    """comm: None, "p2p" (one-rank peer-to-peer comm block) or "rccl" (one-rank communicator)."""
    from emu_amd import synth
    from emu_amd.llama import EmuHipContext, LlamaEngine
    dev = torch.device("cuda", 0)
    real = EmuHipContext(dev, 0, 1)
    if comm == "p2p":
        real.init_tp(lambda b: b, force=True, allgather_bytes=lambda b: [b], rccl=False)
    elif comm == "rccl":
        real.init_tp(lambda b: b, force=True)
    eng = LlamaEngine(cfg, vocab, ShardView(real, tp) if tp > 1 else real)
    eng.load_weights(synth.iter_synth(synth.llama_param_shapes(cfg, vocab), seed=3, device=dev, dtype=BF16))
    return eng, real


def decode_run(eng, mode, S, steps):
    """prefill S random rows, then `steps` greedy steps under set_decode_fused(mode): (ids, hidden after every step)."""
    from emu_amd import ops
    from emu_amd.llama import GreedyState
    eng.set_decode_fused(mode, 0)
    x = rand(1, S, eng.cfg.hidden_size, seed=0)
    hidden, kstart, next_pos = eng.prefill(x, torch.ones(1, S, dtype=torch.long), eng.kv_capacity(S + steps + 8))
    cur = ops.argmax(eng.logits(hidden[:, -1, :].contiguous()), suppress_id=2)
    out = torch.zeros(steps + 2, 1, device=eng.device, dtype=torch.int32)
    st = GreedyState(eng, 1, cur, next_pos, S, kstart, out)
    hs = []
    for _ in range(steps):
        st.step()
        hs.append(st.hidden.clone())
    torch.cuda.synchronize()
    return out.clone(), torch.stack(hs)


def h(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:24]


def dump():
    """one case per line"""
    open(out_path, "w").write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in res.items()) + "\n}\n")


def rec(name, hidden, eng, extra=None, kv=None):
    k, v = kv if kv else (eng.kcache, eng.vcache)
    res[name] = {"hidden": h(hidden), "k": h(k), "v": h(v)}
    if extra:
        res[name].update(extra)
    print(name, res[name], flush=True)
    dump()


def logits_small_ws(eng, rows):
    """emu_llama_logits with no workspace at all: up to 8 rows the head falls back to the bf16 stream with the norm fused."""
    from emu_amd import ops
    from emu_amd._lib import check, lib
    out = torch.empty(rows.shape[0], eng.vocab, device=eng.device, dtype=BF16)
    check(lib().emu_llama_logits(eng.handle, rows.data_ptr(), rows.stride(0), rows.shape[0], out.data_ptr(), out.stride(0), None, 0,
                                 ops.stream(eng.device)), "emu_llama_logits", eng.ctx.handle)
    return out


def profiled(fn):
    """fn() under the weight-stream profiler: (fn's result, {"stream_bytes", "stream_launches"})."""
    from emu_amd._lib import check, lib
    check(lib().emu_profile_gemv(1), "emu_profile_gemv")
    try:
        out = fn()
        torch.cuda.synchronize()
        ms, wb, nl = C.c_double(), C.c_double(), C.c_long()
        check(lib().emu_profile_gemv_read(C.byref(ms), C.byref(wb), C.byref(nl)), "emu_profile_gemv_read")
    finally:
        check(lib().emu_profile_gemv(0), "emu_profile_gemv")
    return out, {"stream_bytes": wb.value, "stream_launches": nl.value}


def step_rows(eng, rows, S, seed, steps=2):
    """a prefill of `rows` prompts of S rows, then `steps` single-token steps of `rows` rows: (every step's residual stream, the
    logits of the last step's rows, the profiler's counters over the steps and the logits call)."""
    dev, H = eng.device, eng.cfg.hidden_size
    eng.release_kv()
    eng.prefill(rand(rows, S, H, seed=seed), torch.ones(rows, S, dtype=torch.long), eng.kv_capacity(S + 8))

    def run():
        outs = []
        for step in range(steps):
            pos = torch.full((rows,), S + step, device=dev, dtype=torch.int32)
            hx = rand(rows, H, seed=seed + 1 + step)
            outs.append(eng.forward(hx, rows, 1, pos, pos.clone(), torch.zeros(rows, device=dev, dtype=torch.int32), ctx=S + step + 1).clone())
        return torch.stack(outs), eng.logits(outs[-1])
    (hs, lg), counters = profiled(run)
    return hs, lg, counters


def rec_logits(name, logits):
    res[name] = {"logits": h(logits)}
    print(name, res[name], flush=True)
    dump()


def want(n):
    return not only or n in only


def rand(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 0.1).to(BF16).cuda()


def main():
    from emu_amd import ops
    from emu_amd._lib import check, lib
    from emu_amd.conf.emu_conf import LlamaCfg
    dev = torch.device("cuda", 0)
    with torch.no_grad():
        if want("main"):
            cfg = LlamaCfg(num_hidden_layers=3)                    # the true LLaMA-33B width
            eng, _ = make_engine(cfg, 2048)
            H = cfg.hidden_size
            # (a) one-row decode steps
            ids, hs = decode_run(eng, 0, 380, 4)
            rec("a_decode_1row", hs, eng, {"ids": h(ids), "logits": h(eng.logits(hs[-1]))})
            # (b) B = 1 prefill, S = 770, with the promise; (c) without
            x = rand(1, 770, H, seed=11)
            m1 = torch.ones(1, 770, dtype=torch.long)
            cap = eng.kv_capacity(800)
            eng.kcache.zero_(); eng.vcache.zero_()
            hid, _, _ = eng.prefill(x, m1, cap)
            rec("b_prefill_770_promise", hid, eng)
            eng.set_prefill_fusion(False)
            eng.kcache.zero_(); eng.vcache.zero_()
            hid, _, _ = eng.prefill(x, m1, cap)
            rec("c_prefill_770_unfused", hid, eng)
            eng.set_prefill_fusion(True)
            # (d) B = 2 left padded
            x2 = rand(2, 300, H, seed=12)
            m2 = torch.ones(2, 300, dtype=torch.long); m2[1, :37] = 0
            hid, kstart, next_pos = eng.prefill(x2, m2, eng.kv_capacity(320))
            rec("d_prefill_B2_leftpad", hid, eng)
            # (e) single-token steps with 5 and with 20 rows (kv_share on, sticky fused norm)
            for B, n in ((1, 5), (4, 5)):
                S = 200
                xb = rand(B, S, H, seed=13 + B)
                hid, kstart, next_pos = eng.prefill(xb, torch.ones(B, S, dtype=torch.long), eng.kv_capacity(S + 16))
                s_max = eng.s_max
                eng.fan_out_kv(B, n, S, s_max)
                rows = B * n
                outs = []
                for step in range(3):
                    hx = rand(rows, H, seed=20 + step)
                    pos = torch.full((rows,), S + step, device=dev, dtype=torch.int32)
                    slot = torch.full((rows,), S + step, device=dev, dtype=torch.int32)
                    ks = torch.zeros(rows, device=dev, dtype=torch.int32)
                    outs.append(eng.forward(hx, rows, 1, pos, slot, ks, ctx=S + step + 1).clone())
                # (the beam cache is allocated without a zero fill: compare the slots the steps wrote)
                extra = {"logits": h(eng.logits(outs[-1]))}
                if rows == 5:
                    extra["logits_small_ws"] = h(logits_small_ws(eng, outs[-1]))
                rec(f"e_beam_rows_{rows}", torch.stack(outs), eng, extra, kv=(eng.kcache[:, :, :, S:S + 3], eng.vcache[:, :, :, S:S + 3]))
                eng.set_kv_share(0, 0)
                eng.release_kv()
            # (i) decode tail, merged o_proj bit (the 33B width is outside gemv_merge_ok: the bit must change nothing here; the
            # wave engine below takes the merge)
            eng.set_decode_tail(True)
            ids, hs = decode_run(eng, 0, 380, 4)
            rec("i_decode_tail", hs, eng, {"ids": h(ids)})
            eng.set_decode_tail(False)
            # (f) fp8 decode with 1 and 2 rows, fp8 prefill
            eng.quantize_fp8()
            eng.use_fp8(True)
            ids, hs = decode_run(eng, 0, 380, 4)
            rec("f_fp8_decode_1row", hs, eng, {"ids": h(ids)})
            xb = rand(2, 100, H, seed=31)
            hid, kstart, next_pos = eng.prefill(xb, torch.ones(2, 100, dtype=torch.long), eng.kv_capacity(116))
            outs = []
            for step in range(3):
                hx = rand(2, H, seed=40 + step)
                pos = torch.full((2,), 100 + step, device=dev, dtype=torch.int32)
                outs.append(eng.forward(hx, 2, 1, pos, pos.clone(), torch.zeros(2, device=dev, dtype=torch.int32), ctx=100 + step + 1).clone())
            rec("f_fp8_decode_2rows", torch.stack(outs), eng, {"logits": h(eng.logits(outs[-1]))})
            eng.use_fp8(True, prefill=True)
            eng.release_kv()
            hid, _, _ = eng.prefill(x, m1, cap)
            rec("f_fp8_prefill_770", hid, eng)
            eng.use_fp8(False)
            del eng
            torch.cuda.empty_cache()
        if want("merge"):
            eng, _ = make_engine(LlamaCfg(**WAVE), 2048)
            lib().emu_gemm_tune(1 << 19)
            ids, hs = decode_run(eng, 0, 250, 12)
            lib().emu_gemm_tune(0)
            rec("i_merged_o_proj", hs, eng, {"ids": h(ids)})
            del eng
        if want("fp4"):
            # (j) the MXFP4 modes on the small shape of tests/test_gpu_fp4*.py (hidden 256, 2 heads, ffn 512, 2 layers; a vocabulary
            # that is no multiple of 64): every row range of every mode, the head with it
            cfg = LlamaCfg(hidden_size=256, intermediate_size=512, num_attention_heads=2, num_hidden_layers=2)
            eng, _ = make_engine(cfg, 2050)
            for tag, mode, row_counts in (("mode1", {}, (1, 2, 5, 16)), ("mode2", {"wide": True}, (1, 2, 5, 16)),
                                          ("mode3", {"wide": True, "all_rows": True}, (17, 20))):
                eng.use_fp4(True, **mode)
                for rows in row_counts:
                    hs, lg, counters = step_rows(eng, rows, 40, seed=50 + rows)
                    if rows == 20:                              # mode 3, 5 rows, no workspace: bf16 while there are bf16 weights
                        counters["logits_5rows_small_ws"] = h(logits_small_ws(eng, hs[-1, :5].contiguous()))
                    rec(f"j_fp4_{tag}_{rows}rows", hs, eng, {"logits": h(lg), **counters},
                        kv=(eng.kcache[:, :, :, 40:42], eng.vcache[:, :, :, 40:42]))
            # a prefill in mode 3 and the same step again after release_bf16
            x = rand(1, 70, cfg.hidden_size, seed=61)

            def prefill_70():
                hid = eng.prefill(x, torch.ones(1, 70, dtype=torch.long), eng.kv_capacity(80))[0]
                return hid, eng.logits(hid.reshape(70, -1).contiguous())
            for tag in ("mode3", "released"):
                eng.release_kv()
                (hid, lg), counters = profiled(prefill_70)
                rec(f"j_fp4_{tag}_prefill_70", hid, eng, {"logits": h(lg), **counters})
                hs, lg, counters = step_rows(eng, 5, 40, seed=70)
                rec(f"j_fp4_{tag}_5rows", hs, eng, {"logits": h(lg), **counters}, kv=(eng.kcache[:, :, :, 40:42], eng.vcache[:, :, :, 40:42]))
                if tag == "mode3":
                    eng.release_bf16()
            del eng
            # (k) the vocabulary-sharded head (emu_llama_set_head_shard) on a 1-rank communicator: rows [64, 1065) of the head, bf16
            # and every MXFP4 head kernel
            eng, real = make_engine(cfg, 2050, comm="rccl")
            check(lib().emu_llama_set_head_shard(eng.handle, 64, 1001), "emu_llama_set_head_shard", eng.ctx.handle)
            for tag, mode in (("bf16", None), ("fp4_mode3", {"wide": True, "all_rows": True})):
                if mode:
                    eng.use_fp4(True, **mode)
                for rows in (1, 5, 20):
                    rec_logits(f"k_head_shard_{tag}_{rows}rows", eng.logits(rand(rows, cfg.hidden_size, seed=80 + rows)))
            del eng, real
            torch.cuda.empty_cache()
        if want("fp8w"):
            # (l) the fp8 modes 3, 5 and 6 on a shape whose three widths are multiples of 256: the few-row stream, the W8A16 GEMM and
            # the bf16 / W8A8 GEMM above it, each followed by the head -- first without its fp8 copy (bf16), then with
            cfg = LlamaCfg(hidden_size=256, intermediate_size=512, num_attention_heads=2, num_hidden_layers=3)
            eng, _ = make_engine(cfg, 2050)
            eng._fp8 = {}                                       # the layers' copies only: quantize_fp8 adds the head's
            for i in range(cfg.num_hidden_layers):
                a = []
                for k in ("wqkv", "wo", "wgu", "wdown"):
                    eng._fp8[f"{i}.{k}"] = ops.quantize_fp8_rows(eng._keep[f"{i}.{k}"])
                    a += [t.data_ptr() for t in eng._fp8[f"{i}.{k}"]]
                check(lib().emu_llama_set_layer_fp8(eng.handle, i, *a), "emu_llama_set_layer_fp8", eng.ctx.handle)
            for head in ("no_head_copy", "head_copy"):
                if head == "head_copy":
                    old, eng._fp8 = eng._fp8, None              # (kept until every pointer is registered anew)
                    eng.quantize_fp8()
                    del old
                for tag, mode in (("mode3", dict(wide=True)), ("mode5", dict(wide=True, mid=True)), ("mode6", dict(prefill=True, wide=True, mid=True))):
                    eng.use_fp8(True, **mode)
                    for rows in (5, 20, 65):
                        hs, lg, counters = step_rows(eng, rows, 40, seed=90 + rows)
                        if rows == 5:                           # no workspace: the bf16 stream with the norm fused
                            counters["logits_small_ws"] = h(logits_small_ws(eng, hs[-1]))
                        rec(f"l_fp8_{head}_{tag}_{rows}rows", hs, eng, {"logits": h(lg), **counters},
                            kv=(eng.kcache[:, :, :, 40:42], eng.vcache[:, :, :, 40:42]))
            del eng
            torch.cuda.empty_cache()
        if want("pack"):
            # (m) the 13-bit packed streams on the shape of tests/test_gpu_bf16_pack_wide.py (its sets are made under emu_gemm_tune bit
            # 17): the one-row and the few-row switch, under the default L2-warm mask, with the decode tail, and with no warming
            cfg = LlamaCfg(hidden_size=256, intermediate_size=512, num_attention_heads=2, num_hidden_layers=2)
            eng, _ = make_engine(cfg, 1024)
            lib().emu_gemm_tune(1 << 17)
            try:
                eng.pack_bf16(tune=1 << 17)
                eng.use_bf16_pack(True)
                for tag, setup in (("default", lambda: None), ("tail", lambda: eng.set_decode_tail(True)), ("no_warm", lambda: eng.set_l2_warm(0))):
                    setup()
                    for wide in (False, True):
                        eng.use_bf16_pack_wide(wide)
                        for rows in (1, 5, 16):
                            hs, lg, counters = step_rows(eng, rows, 24, seed=110 + rows)
                            rec(f"m_pack_{tag}_wide{int(wide)}_{rows}rows", hs, eng, {"logits": h(lg), **counters},
                                kv=(eng.kcache[:, :, :, 24:26], eng.vcache[:, :, :, 24:26]))
                    eng.set_decode_tail(False)
            finally:
                lib().emu_gemm_tune(0)
            del eng
            torch.cuda.empty_cache()
        if want("fused"):
            # (g) modes 1, 2, 3 on the TP = 8 shard emulation, mode 4 on the TP = 4 one
            eng, _ = make_engine(LlamaCfg(num_hidden_layers=2), 2048, tp=8, comm="p2p")
            for mode in (0, 1, 2, 3):
                f0 = eng.decode_fused_stats()[1]
                ids, hs = decode_run(eng, mode, 200, 5)
                g, f1 = eng.decode_fused_stats()
                rec(f"g_tp8_mode{mode}", hs, eng, {"ids": h(ids), "fused_forwards": f1 - f0, "giveups": g})
            eng.set_decode_fused(0)
            eng.ctx.check_p2p()
            del eng
            cfg = LlamaCfg(hidden_size=4096, intermediate_size=4 * 2048, num_attention_heads=4 * 8, num_hidden_layers=3)
            eng, _ = make_engine(cfg, 1024, tp=4, comm="p2p")
            for mode in (0, 4):
                f0 = eng.decode_fused_stats()[1]
                ids, hs = decode_run(eng, mode, 250, 10)
                g, f1 = eng.decode_fused_stats()
                rec(f"g_tp4_mode{mode}", hs, eng, {"ids": h(ids), "fused_forwards": f1 - f0, "giveups": g})
            eng.set_decode_fused(0)
            del eng
            torch.cuda.empty_cache()
        for comm, tp, S in (("p2p", 8, 1544), ("rccl", 8, 1544), ("p2p", 4, 1544), ("p2p", 2, 1100)):
            if not want("lanes"):
                break
            # (h) the two-lane schedule as tests/test_gpu_tp_overlap.py drives it (TP = 2: 26 heads, the RoPE epilogue in both lanes;
            # TP = 4 / 8 shards: 13 / 7 heads, the rope_kv + transpose_v sequence)
            cfg = LlamaCfg(num_hidden_layers=2)
            eng, real = make_engine(cfg, 2048, tp=tp, comm=comm)
            x = rand(1, S, cfg.hidden_size, seed=7)
            mask = torch.ones(1, S, dtype=torch.long, device=dev)
            cap = eng.kv_capacity(S + 8)
            eng.set_tp_overlap(1024)
            n0 = eng.tp_overlap_count()
            hid, _, _ = eng.prefill(x, mask, cap)
            rec(f"h_two_lane_tp{tp}_{comm}", hid, eng, {"overlap_forwards": eng.tp_overlap_count() - n0})
            eng.set_tp_overlap(0)
            hid, _, _ = eng.prefill(x, mask, cap)
            rec(f"h_serial_tp{tp}_{comm}", hid, eng, {"overlap_forwards": eng.tp_overlap_count() - n0 - 1})
            if comm == "p2p":
                real.check_p2p()
            del eng, real
            torch.cuda.empty_cache()
    print("EQUIV DONE", flush=True)


if __name__ == "__main__":
    main()
