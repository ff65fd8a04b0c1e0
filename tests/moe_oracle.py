"""fp32 restatement of the Mixtral sparse-MoE decoder (test infrastructure).  HF transformers 5.15,
models/mixtral/modeling_mixtral.py:
  MixtralTopKRouter.forward (:104-111): logits = h Wr^T, softmax in fp32, topk, weights / sum(weights)
  MixtralExperts.forward (:69-93): per hit expert, silu(gate) * up -> down, * routing weight, index_add_ over the tokens
  MixtralSparseMoeBlock.forward (:122-130), MixtralDecoderLayer (attention of Mistral, post_attention_layernorm -> MoE)
Attention, RoPE and RMSNorm come from oracle.vl2_oracle (the Mistral path), so only the MoE block is restated here."""
import torch
import torch.nn.functional as F

from oracle import vl2_oracle as O


def small_mixtral_cfg(num_frames=4, n_layers=2, E=8, k=2):
    """Tiny VideoLLaMA2-8x7B-shaped config (CLIP-small + stc + a Mixtral of `n_layers`) on the kernels' granularity."""
    cfg = O.config_small(num_frames)
    cfg["llm"] = dict(cfg["llm"], family="mixtral", num_hidden_layers=n_layers, num_local_experts=E, num_experts_per_tok=k)
    return cfg


def moe_names(cfg):
    """(name, shape) of the MoE parameters of every layer, transformers >= 5 layout."""
    l = cfg["llm"]
    E, D, I = l["num_local_experts"], l["hidden_size"], l["intermediate_size"]
    out = []
    for i in range(l["num_hidden_layers"]):
        p = f"model.layers.{i}."
        out += [(p + "mlp.gate.weight", (E, D)), (p + "mlp.experts.gate_up_proj", (E, 2 * I, D)), (p + "mlp.experts.down_proj", (E, D, I))]
    return out


def structured_router(name, shape, seed, scale):
    """A seeded router whose top-k calls are decidable: every expert row is c_e * u plus a little noise, u one seeded unit direction and
    c a seeded permutation of scale * (3, 2.975, 0.3, 0.1, -0.1, -0.3, -2.975, -3) (E = 8; other E: evenly spaced).  A token whose
    projection z on u is clear of 0 then has its top 2 (c = 3, 2.975 for z > 0; -3, -2.975 for z < 0) close to each other and far above
    the third, so the top-2 / top-3 probability margin is large; only |z| below ~2 / scale is ambiguous."""
    E, D = shape
    u = O.seeded_tensor(name + ".u", (D,), seed)
    u = u / u.norm()
    c = torch.tensor([3, 2.975, 0.3, 0.1, -0.1, -0.3, -2.975, -3]) if E == 8 else torch.linspace(3, -3, E)
    g = torch.Generator().manual_seed(int.from_bytes(name.encode()[-8:], "little") ^ seed)
    c = c[torch.randperm(E, generator=g)]
    return scale * c[:, None] * u[None, :] + 0.05 * O.seeded_tensor(name, shape, seed)


def seeded_state_dict(cfg, seed=1234, router_scale=1.0, structured=False):
    """The Mistral path's seeded weights (oracle.vl2_oracle) with every MLP replaced by a MoE block: expert matrices drawn per expert
    (fan-in = their input width), rounded once to bf16.  router_scale widens the router logits (clearer top-k margins); structured=True
    draws the router with structured_router (decidable routing for golden fixtures)."""
    dense = {n for n in ("mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")}
    sd = {k: v for k, v in O.seeded_state_dict(cfg, seed).items() if not any(k.endswith(d) for d in dense)}
    for name, shape in moe_names(cfg):
        if name.endswith("gate.weight"):
            t = structured_router(name, shape, seed, router_scale) if structured else router_scale * O.seeded_tensor(name, shape, seed)
        else:
            t = torch.stack([O.seeded_tensor(f"{name}.{e}", shape[1:], seed) for e in range(shape[0])])
        sd[name] = t.bfloat16().float()
    return sd


def to_v4_keys(sd, cfg):
    """The same weights under the transformers 4.x names (block_sparse_moe.gate, experts.{e}.w1 / w3 / w2)."""
    l = cfg["llm"]
    I = l["intermediate_size"]
    out = {}
    for k, v in sd.items():
        if ".mlp.gate.weight" in k:
            out[k.replace(".mlp.gate.", ".block_sparse_moe.gate.")] = v
        elif ".mlp.experts.gate_up_proj" in k:
            p = k.replace("mlp.experts.gate_up_proj", "block_sparse_moe.experts.")
            for e in range(v.shape[0]):
                out[f"{p}{e}.w1.weight"] = v[e, :I].clone()
                out[f"{p}{e}.w3.weight"] = v[e, I:].clone()
        elif ".mlp.experts.down_proj" in k:
            p = k.replace("mlp.experts.down_proj", "block_sparse_moe.experts.")
            for e in range(v.shape[0]):
                out[f"{p}{e}.w2.weight"] = v[e].clone()
        else:
            out[k] = v
    return out


def route(h, wr, k):
    """MixtralTopKRouter.forward on normalised rows h [S, D]: (ids [S, k], weights [S, k], probs [S, E]).  torch.topk breaks ties toward
    the lower index on these sizes, as the kernel does."""
    p = F.softmax(F.linear(h, wr).float(), dim=-1)
    w, ids = torch.topk(p, k, dim=-1)
    return ids, w / w.sum(-1, keepdim=True), p


def margins(probs, k):
    """Top-k / top-(k+1) probability gap of every row (how decidable the routing is)."""
    top = probs.topk(min(k + 1, probs.shape[-1]), dim=-1).values
    return top[:, k - 1] - top[:, k] if top.shape[-1] > k else torch.full_like(top[:, 0], float("inf"))


def moe_block(sd, cfg, i, x1, ids=None, follow_below=None):
    """x1 [S, D] -> MoE(RMSNorm(x1)) [S, D] (without the residual).  ids: optional [S, k] expert choice to use instead of the router's
    (to follow a kernel's choice on rows the bf16 floor cannot decide); the weights are the router's probabilities of those experts,
    renormalised."""
    l = cfg["llm"]
    p = f"model.layers.{i}."
    I, k = l["intermediate_size"], l["num_experts_per_tok"]
    h = O.rmsnorm(x1, sd[p + "post_attention_layernorm.weight"], l["rms_norm_eps"])
    rid, w, probs = route(h, sd[p + "mlp.gate.weight"], k)
    if ids is not None:
        if follow_below is not None:           # the kernel's choice only where the fp32 routing is this close to a tie
            rid = torch.where((margins(probs, k) < follow_below)[:, None], ids.long().to(rid.device), rid)
        else:
            rid = ids.long().to(rid.device)
        pw = probs.gather(1, rid)
        w = pw / pw.sum(-1, keepdim=True)
    gu, dn = sd[p + "mlp.experts.gate_up_proj"], sd[p + "mlp.experts.down_proj"]
    y = torch.zeros_like(x1)
    for e in range(gu.shape[0]):                     # MixtralExperts.forward: per expert, tokens in ascending order
        pos, tok = torch.where((rid == e).T)
        if tok.numel() == 0:
            continue
        g, u = F.linear(h[tok], gu[e]).chunk(2, dim=-1)
        out = F.linear(F.silu(g) * u, dn[e]) * w[tok, pos, None]
        y.index_add_(0, tok, out.to(y.dtype))
    return y


def mixtral_layer(sd, cfg, i, x, cos, sin, kv=None, ids=None, follow_below=None):
    """MixtralDecoderLayer.forward for one sequence: the Mistral attention (vl2_oracle.mistral_layer without its MLP) + the MoE block."""
    l = cfg["llm"]
    nh, nkv, hd, eps = l["num_attention_heads"], l["num_key_value_heads"], l["head_dim"], l["rms_norm_eps"]
    p = f"model.layers.{i}."
    S = x.shape[0]
    h = O.rmsnorm(x, sd[p + "input_layernorm.weight"], eps)
    q = F.linear(h, sd[p + "self_attn.q_proj.weight"]).view(S, nh, hd).transpose(0, 1)
    k = F.linear(h, sd[p + "self_attn.k_proj.weight"]).view(S, nkv, hd).transpose(0, 1)
    v = F.linear(h, sd[p + "self_attn.v_proj.weight"]).view(S, nkv, hd).transpose(0, 1)
    q = q * cos + O.rotate_half(q) * sin
    k = k * cos + O.rotate_half(k) * sin
    if kv is not None:
        k = torch.cat([kv[0], k], 1)
        v = torch.cat([kv[1], v], 1)
    Sk = k.shape[1]
    rep = nh // nkv
    kk = k[:, None].expand(nkv, rep, Sk, hd).reshape(nh, Sk, hd)
    vv = v[:, None].expand(nkv, rep, Sk, hd).reshape(nh, Sk, hd)
    a = torch.matmul(q, kk.transpose(1, 2)) * (hd ** -0.5)
    qpos = torch.arange(Sk - S, Sk, device=x.device)[:, None]
    a = a.masked_fill((torch.arange(Sk, device=x.device)[None, :] > qpos)[None], torch.finfo(a.dtype).min)
    a = F.softmax(a, dim=-1, dtype=torch.float32).to(q.dtype)
    o = torch.matmul(a, vv).transpose(0, 1).reshape(S, nh * hd)
    x = x + F.linear(o, sd[p + "self_attn.o_proj.weight"])
    return x + moe_block(sd, cfg, i, x, ids, follow_below), (k, v)


def mixtral_forward(sd, cfg, x, start_pos=0, caches=None, last_only=True):
    """MixtralModel.forward + lm_head for new embeddings x [S, D] at positions start_pos...  Returns (logits, caches)."""
    l = cfg["llm"]
    S = x.shape[0]
    cos, sin = O.rope_cos_sin(cfg, torch.arange(start_pos, start_pos + S), x.dtype)
    cos, sin = cos.to(x.device), sin.to(x.device)
    new = []
    for i in range(l["num_hidden_layers"]):
        x, kv = mixtral_layer(sd, cfg, i, x, cos, sin, None if caches is None else caches[i])
        new.append(kv)
    x = O.rmsnorm(x, sd["model.norm.weight"], l["rms_norm_eps"])
    if last_only:
        x = x[-1:]
    return F.linear(x, sd["lm_head.weight"]), new


def fixture_state_dict(g):
    """The weights of a golden fixture minted by scripts/make_golden_mixtral.py (rebuilt from its seed, never stored)."""
    return seeded_state_dict(g["cfg"], g["seed"], router_scale=g["router_scale"], structured=g.get("structured_router", False))


def write_mixtral_checkpoint(path, g):
    """A local VideoLLaMA2-8x7B-shaped checkpoint directory (config.json of type videollama2_mixtral with its expert counts,
    vision_config.json, model.safetensors in bf16) holding the fixture's weights, as api.model_init reads it.  Returns the HF dict."""
    import json
    import os
    from safetensors.torch import save_file
    cfg = g["cfg"]
    v, l = cfg["vision"], cfg["llm"]
    sd = {k: t.bfloat16().contiguous() for k, t in fixture_state_dict(g).items()}
    save_file(sd, os.path.join(str(path), "model.safetensors"))
    hf = dict(model_type="videollama2_mixtral", hidden_size=l["hidden_size"], intermediate_size=l["intermediate_size"],
              num_hidden_layers=l["num_hidden_layers"], num_attention_heads=l["num_attention_heads"],
              num_key_value_heads=l["num_key_value_heads"], head_dim=l["head_dim"], vocab_size=l["vocab_size"],
              rms_norm_eps=l["rms_norm_eps"], rope_theta=l["rope_theta"], sliding_window=None, max_position_embeddings=32768,
              num_local_experts=l["num_local_experts"], num_experts_per_tok=l["num_experts_per_tok"], num_frames=cfg["num_frames"],
              mm_vision_tower="somewhere/clip-synthetic", mm_projector_type="stc_connector", mm_vision_select_layer=v["select_layer"])
    json.dump(hf, open(os.path.join(str(path), "config.json"), "w"))
    json.dump({k: v[k] for k in v if k != "select_layer"}, open(os.path.join(str(path), "vision_config.json"), "w"))
    return hf
