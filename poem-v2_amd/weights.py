"""Checkpoint surface of the path: the reference's ``state_dict`` key names (relative to the head, i.e. without the
``ptEmb_head.`` prefix of the full-model checkpoint) for the tensors the forward actually reads, their shapes,
and a seeded generator used wherever real checkpoints are unavailable (bench, tests, golden vectors).

Key names follow SURVEY.md section 8b / the reference modules:
  ptEmb_head.py:94,101,701-707,729  (input_proj, adapt_pos3d, merge_net_feature, query_feat_embedding)
  pt_metro_transformer.py:25-31,49-54,113,125-126  (reg_branch, attn/cross_attn, embedding, flat_verts, mano_linear)
  point_transformers.py:49-56,101-108  (fc1, fc2, fc_delta, fc_gamma, w_qs, w_ks, w_vs)
Dead tensors the reference also serialises (center_shift_layer, reg_branches, position_encoder, BERT word
embeddings, pooler, ...) are accepted and ignored by ``split_state_dict``; ``is_dead_reference_key`` names
them one by one, and ``StrictLoadFilter`` lets a plain ``load_state_dict(strict=True)`` swallow exactly those."""
import zlib
from collections import OrderedDict

import torch

MODEL_EMBED = {"small": 128, "medium": 256, "large": 512, "huge": 1024, "medium_MANO": 256}


def live_key_shapes(embed, in_channels=160, nquery=799, nblocks=3, parametric=False, petr=False, depth_num=32):
    C = embed
    k = OrderedDict()

    def lin(name, o, i, bias=True):
        k[name + ".weight"] = (o, i)
        if bias:
            k[name + ".bias"] = (o,)

    k["input_proj.weight"] = (C, in_channels, 1, 1)
    k["input_proj.bias"] = (C,)
    k["adapt_pos3d.weight"] = (C, 3 * C // 2, 1, 1)
    k["adapt_pos3d.bias"] = (C,)
    lin("merge_net_feature.0.0", C, C)
    lin("merge_net_feature.0.2", C // 2, C)
    lin("merge_net_feature.1.0", C // 2, C // 2)
    lin("merge_net_feature.1.2", C, C // 2)
    k["query_feat_embedding.weight"] = (nquery, C)
    for i in range(nblocks):
        p = f"transformer.pt_metro_encoder.{i}."
        lin(p + "embedding", C, C)
        for a in ("attn", "cross_attn"):
            for n in ("query", "key", "value"):
                lin(p + f"encoder.{a}.self.{n}", C, C)
            lin(p + f"encoder.{a}.output.dense", C, C)
            k[p + f"encoder.{a}.output.LayerNorm.weight"] = (C,)
            k[p + f"encoder.{a}.output.LayerNorm.bias"] = (C,)
        for a in ("query_self_attn", "query_cross_attn"):
            q = p + f"encoder.vec_attn.{a}."
            lin(q + "fc1", C, C)
            lin(q + "fc2", C, C)
            lin(q + "fc_delta.0", C, 3)
            lin(q + "fc_delta.2", C, C)
            lin(q + "fc_gamma.0", C, C)
            lin(q + "fc_gamma.2", C, C)
            lin(q + "w_qs", C, C, bias=False)
            lin(q + "w_ks", C, C, bias=False)
            lin(q + "w_vs", C, C, bias=False)
        lin(p + "encoder.vec_attn.reg_branch.0", C, C)
        lin(p + "encoder.vec_attn.reg_branch.2", 3, C)
        lin(p + "encoder.intermediate.dense", 4 * C, C)
        lin(p + "encoder.output.dense", C, 4 * C)
        k[p + "encoder.output.LayerNorm.weight"] = (C,)
        k[p + "encoder.output.LayerNorm.bias"] = (C,)
        if parametric:
            lin(p + "flat_verts", 1, nquery)
            lin(p + "mano_linear", 106, C)
    if petr:
        # PETR_EMBEDDING=True (ptEmb_head.py:101-105,865-867): position_encoder is live.  Listed LAST (after the blocks, not at
        # its state_dict position behind adapt_pos3d) so that the canonical indices of every other tensor do not depend on it.
        k["position_encoder.0.weight"] = (2 * C, 3 * depth_num, 1, 1)
        k["position_encoder.0.bias"] = (2 * C,)
        k["position_encoder.2.weight"] = (C, 2 * C, 1, 1)
        k["position_encoder.2.bias"] = (C,)
    return k


def seeded_state_dict(embed, seed=0, gain=1.0, ln_spread=0.02, **kw):
    """Deterministic, well-conditioned weights: every tensor is drawn from its own CPU generator seeded by
    (seed, crc32(key)), so the reference module and this build can be filled identically without shipping blobs.

    Scales follow the reference's initialisers: N(0, 0.02) for every Linear inside a decoder block (BERT v4
    ``init_weights``, applied by point_METRO_block to all sub-modules), U(+-1/sqrt(fan_in)) for head-level
    Linear/Conv, N(0,1) for the query embedding; biases and LayerNorm offsets get small non-zero values so that
    every term of the arithmetic is exercised.  ``gain`` scales the block weights and ``ln_spread`` the deviation of the
    LayerNorm gains from 1 ("hot" stress variant: with gain 1 the coordinate update of a block is ~1e-3 normalised units, so
    attention-path error is attenuated ~1000x before it reaches a vertex and the neighbour sets of blocks 1, 2 are
    essentially the template's; gain 2.5 makes activations, updates and neighbour changes O(1) -- the conditioning of a
    trained checkpoint, tests/golden/*_hot.npz)."""
    out = OrderedDict()
    for key, shape in live_key_shapes(embed, **kw).items():
        g = torch.Generator().manual_seed((seed * 1000003 + zlib.crc32(key.encode())) & 0x7FFFFFFF)
        in_block = key.startswith("transformer.")
        if key.endswith("LayerNorm.weight"):
            t = 1.0 + ln_spread * torch.randn(shape, generator=g)
        elif key.endswith("LayerNorm.bias"):
            t = 0.02 * torch.randn(shape, generator=g)
        elif key == "query_feat_embedding.weight":
            t = torch.randn(shape, generator=g)
        elif in_block:
            t = 0.02 * gain * torch.randn(shape, generator=g)
            if "fc_delta.0.weight" in key:       # 3 -> C layer acts on O(1) coordinates
                t = t * 10.0
        else:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            bound = 1.0 / (fan_in ** 0.5) if len(shape) > 1 else 0.05
            t = (torch.rand(shape, generator=g) * 2 - 1) * bound
        out[key] = t.float().contiguous()
    return out


def split_state_dict(sd, embed, strip_prefixes=("module.", "ptEmb_head."), **kw):
    """Pick the live tensors out of a reference checkpoint ``state_dict`` (full-model or head-only); tolerate dead
    and unexpected keys (the reference loads with strict=True, the dead tensors are simply unused)."""
    want = live_key_shapes(embed, **kw)
    norm = {}
    for key, val in sd.items():
        k = key
        changed = True
        while changed:
            changed = False
            for p in strip_prefixes:
                if k.startswith(p):
                    k = k[len(p):]
                    changed = True
        norm[k] = val
    live, missing = OrderedDict(), []
    for key, shape in want.items():
        if key not in norm:
            missing.append(key)
            continue
        t = torch.as_tensor(norm[key]).float()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{key}: checkpoint shape {tuple(t.shape)} != expected {tuple(shape)}")
        live[key] = t.contiguous()
    if missing:
        raise KeyError(f"checkpoint lacks {len(missing)} live tensors, e.g. {missing[:4]}")
    ignored = sorted(set(norm) - set(want))
    return live, ignored


# ---- the reference head's dead surface: what a strict load may swallow --------------------------------------
# Rule table: key pattern relative to the head -> shape.  "#" in a pattern is a decimal index below a bound of the configuration
# (a block: N_BLOCKS; a reg_branches entry: NUM_PREDS); in a shape, C = EMBED_DIMS, P = POINTS_FEAT_DIM, Q = NUM_QUERY,
# D = 3 * DEPTH_NUM, None = any positive extent (the three BERT embedding tables: their row counts come from
# config/backbone/bert_cfg.json and the transformer node upstream, not from the head's config).
_BLOCK = "transformer.pt_metro_encoder.#."
_REG_BRANCH = "reg_branches.#."
_DEAD_RULES = (
    ("center_shift_layer.0.weight", ("Q", "Q")), ("center_shift_layer.0.bias", ("Q",)),           # ptEmb_head.py:87-88
    ("center_shift_layer.2.weight", (1, "Q")), ("center_shift_layer.2.bias", (1,)),
    (_REG_BRANCH + "0.weight", ("P", "P")), (_REG_BRANCH + "0.bias", ("P",)),                     # :95-99, one per NUM_PREDS
    (_REG_BRANCH + "2.weight", (3, "P")), (_REG_BRANCH + "2.bias", (3,)),
    ("reference_embed.weight", ("Q", "C")),                                                       # :107
    ("query_embedding.0.weight", ("C", "C")), ("query_embedding.0.bias", ("C",)),                 # :722-726
    ("query_embedding.2.weight", ("P", "C")), ("query_embedding.2.bias", ("P",)),
    ("merge_net_query_feature.0.0.weight", ("C", "C")), ("merge_net_query_feature.0.0.bias", ("C",)),          # :711-717
    ("merge_net_query_feature.0.2.weight", ("C/2", "C")), ("merge_net_query_feature.0.2.bias", ("C/2",)),
    ("merge_net_query_feature.1.0.weight", ("C/2", "C/2")), ("merge_net_query_feature.1.0.bias", ("C/2",)),
    ("merge_net_query_feature.1.2.weight", ("C", "C/2")), ("merge_net_query_feature.1.2.bias", ("C",)),
    ("layer_global_feat.weight", ("C", 512)), ("layer_global_feat.bias", ("C",)),                 # :719
    (_BLOCK + "embeddings.word_embeddings.weight", (None, "C")),                                  # pt_metro_transformer.py:102-106
    (_BLOCK + "embeddings.position_embeddings.weight", (None, "C")),
    (_BLOCK + "embeddings.token_type_embeddings.weight", (None, "C")),
    (_BLOCK + "embeddings.LayerNorm.weight", ("C",)), (_BLOCK + "embeddings.LayerNorm.bias", ("C",)),
    (_BLOCK + "pooler.dense.weight", ("C", "C")), (_BLOCK + "pooler.dense.bias", ("C",)),
    (_BLOCK + "position_embeddings.weight", (None, "C")),
)
# position_encoder (ptEmb_head.py:102-106) is dead unless PETR_EMBEDDING makes it live
_DEAD_RULES_NO_PETR = (
    ("position_encoder.0.weight", ("2C", "D", 1, 1)), ("position_encoder.0.bias", ("2C",)),
    ("position_encoder.2.weight", ("C", "2C", 1, 1)), ("position_encoder.2.bias", ("C",)),
)
# Buffers a real manotorch ManoLayer would serialise under the head (ptEmb_head.py:732) and, with PARAMETRIC_OUTPUT, under every
# block (pt_metro_transformer.py:120).  UNPINNED: manotorch is absent wherever this is built and tested, dropin.json was recorded
# without it and so lists none of these keys; the names are restated from manotorch's published source and no fixture or test
# holds them to a real manotorch.  Their shapes (asset dependent) are not checked.
_MANOTORCH_BUFFERS = ("th_betas", "th_shapedirs", "th_posedirs", "th_v_template", "th_J_regressor", "th_weights", "th_faces",
                      "th_hands_mean", "th_comps", "th_selected_comps")


def _match_pattern(pattern, key):
    """``key`` against a "#"-pattern -> the tuple of indices it carries, or None."""
    pp, kp = pattern.split("."), key.split(".")
    if len(pp) != len(kp):
        return None
    idx = []
    for a, b in zip(pp, kp):
        if a == "#":
            if not (b.isdigit() and str(int(b)) == b):
                return None
            idx.append(int(b))
        elif a != b:
            return None
    return tuple(idx)


def is_dead_reference_key(key, embed, shape=None, in_channels=160, nquery=799, nblocks=3, parametric=False, petr=False,
                          depth_num=32, pt_feat_dim=None, num_preds=3):
    """Does ``key`` (relative to the head, as in :func:`live_key_shapes`) name a tensor of the reference head's DEAD surface --
    one upstream's ``POEM_Generalized_Head`` allocates and serialises but whose value its forward never reads?

    The answer comes from a closed rule table held to ``tests/golden/dropin.json`` (every key of the reference head with its
    shape), never from "a key this build does not know": an invented or misspelt name is not dead, a block index at or past
    ``nblocks`` is not dead, and no live key is.  ``shape`` is the checkpoint tensor's shape; ``None`` asks about the name only.
    A dead NAME whose shape is not the one the reference's constructor gives it for this configuration raises ``ValueError``:
    such a tensor comes from another model size, and a checkpoint of another size must not load quietly.  (The strict-load hook
    of the head turns that into torch's own "Unexpected key(s)" error naming the key: it leaves the key unswallowed.)"""
    C, P = int(embed), int(embed if pt_feat_dim is None else pt_feat_dim)
    dims = {"C": C, "2C": 2 * C, "C/2": C // 2, "P": P, "Q": int(nquery), "D": 3 * int(depth_num)}
    for pattern, want in _DEAD_RULES + (() if petr else _DEAD_RULES_NO_PETR):
        idx = _match_pattern(pattern, key)
        if idx is None:
            continue
        if pattern.startswith(_BLOCK) and idx[0] >= nblocks:
            return False
        if pattern.startswith(_REG_BRANCH) and idx[0] >= num_preds:
            return False
        if shape is not None:
            want = tuple(dims.get(d, d) for d in want)
            got = tuple(int(v) for v in shape)
            if len(got) != len(want) or any(g != w if w is not None else g < 1 for g, w in zip(got, want)):
                raise ValueError(f"{key}: a dead tensor of the reference head, but of shape {got} where this configuration's "
                                 f"reference has {tuple('*' if w is None else w for w in want)}")
        return True
    holder, _, leaf = key.rpartition(".")
    if leaf in _MANOTORCH_BUFFERS:
        if holder == "mano_layer":
            return True
        idx = _match_pattern(_BLOCK + "mano_layer", holder) if parametric else None
        return idx is not None and idx[0] < nblocks
    return False


class StrictLoadFilter:
    """The two hooks that let ``load_state_dict(strict=True)`` accept a reference checkpoint on a module of this package
    (``POEM_Generalized_Head``, ``PtEmbedTRv4``), as the root of the call or as a child under any prefix: the pre hook notes
    the prefix torch hands the module and the shapes of the keys below it, the post hook takes exactly the dead keys
    (:func:`is_dead_reference_key`) out of ``incompatible_keys.unexpected_keys``.  Everything else -- unknown names, missing live
    keys, shape mismatches of live keys -- is reported as torch reports it.  ``rel_prefix`` places the module inside the head
    ("" for the head, "transformer." for the decoder); ``classify_kw`` returns the keyword arguments of the classifier."""

    def __init__(self, module, rel_prefix, classify_kw, on_swallowed):
        self.rel_prefix, self.classify_kw, self.on_swallowed = rel_prefix, classify_kw, on_swallowed
        self._prefix, self._shapes = "", {}
        pre = getattr(module, "register_load_state_dict_pre_hook", None)
        if pre is not None:
            pre(self._pre)
        else:                                                      # torch < 2.5: the private spelling of the same hook
            module._register_load_state_dict_pre_hook(self._pre, with_module=True)
        module.register_load_state_dict_post_hook(self._post)

    def _pre(self, module, state_dict, prefix, *unused):
        self._prefix = prefix
        self._shapes = {k: tuple(getattr(v, "shape", ())) for k, v in state_dict.items() if k.startswith(prefix)}

    def _post(self, module, incompatible_keys):
        prefix, shapes = self._prefix, self._shapes
        self._prefix, self._shapes = "", {}
        kw = self.classify_kw()
        embed = kw.pop("embed")
        swallowed, keep = [], []
        for key in incompatible_keys.unexpected_keys:
            dead = False
            if key.startswith(prefix) and key in shapes:
                try:
                    dead = is_dead_reference_key(self.rel_prefix + key[len(prefix):], embed, shape=shapes[key], **kw)
                except ValueError:
                    dead = False                                   # a dead name of the wrong shape stays "unexpected"
            (swallowed if dead else keep).append(key)
        incompatible_keys.unexpected_keys[:] = keep
        self.on_swallowed([k[len(prefix):] for k in swallowed])


# ---- convolutional glue in front of the head (poem_v2_amd.decode) ----------------------------------
_FEAT_SIZE = (40, 80, 160, 320)          # lib/models/POEM.py:55-56 upstream (HRNet)


def decoder_key_shapes(backbone="HRNet"):
    """state_dict keys (relative to the model) and shapes of feat_delayer / feat_in / uv_delayer / uv_out
    (lib/models/POEM.py:59-112 upstream) for the pyramid of ``backbone`` ("HRNet" | "resnet18" | "resnet34" | "resnet50")."""
    f = {"HRNet": _FEAT_SIZE, "resnet18": (64, 128, 256, 512), "resnet34": (64, 128, 256, 512),
         "resnet50": (256, 512, 1024, 2048)}[backbone]
    ks = {}

    def block(name, cin, cout, k, norm):
        ks[f"{name}.conv.weight"] = (cout, cin, k, k)
        ks[f"{name}.conv.bias"] = (cout,)
        if norm:
            for n in ("weight", "bias", "running_mean", "running_var"):
                ks[f"{name}.norm.{n}"] = (cout,)

    if backbone != "HRNet":                                  # POEM.py:59-86: both stacks go up from the coarsest level
        for stack in ("feat_delayer", "uv_delayer"):
            for i in range(3):
                block(f"{stack}.{i}", f[3 - i] + f[2 - i], f[2 - i], 3, True)
        block("feat_in", f[0], f[1], 1, False)
        block("uv_out", f[0], 21, 1, False)
        return ks
    for i in range(3):
        block(f"feat_delayer.{i}", f[i], f[i + 1], 3, True)
    block("feat_in", f[3], f[2], 1, False)
    block("uv_delayer.0", f[3] + f[2], f[2], 3, True)
    block("uv_delayer.1", f[2] + f[1], f[1], 3, True)
    block("uv_delayer.2", f[1] + f[0], f[0], 3, True)
    block("uv_out", f[0], 21, 1, False)
    return ks


def seeded_decoder_state_dict(seed=0, backbone="HRNet"):
    """Deterministic weights for fixtures / benches: conv weights N(0, sqrt(2 / fan_out)) as ConvBlock's
    kaiming_normal_(mode='fan_out') draws them (lib/models/bricks/conv.py:31-33 upstream), small random biases, and
    *non-trivial* BatchNorm statistics so that the folded affine is exercised (the reference initialises gamma = 1,
    beta = 0, mean = 0, var = 1)."""
    g = torch.Generator().manual_seed(1000 + seed)
    sd = {}
    for k, shp in decoder_key_shapes(backbone).items():
        if k.endswith("conv.weight"):
            fan_out = shp[0] * shp[2] * shp[3]
            sd[k] = torch.randn(shp, generator=g) * (2.0 / fan_out) ** 0.5
        elif k.endswith("conv.bias"):
            sd[k] = 0.05 * torch.randn(shp, generator=g)
        elif k.endswith("norm.weight"):
            sd[k] = 1.0 + 0.2 * torch.randn(shp, generator=g)
        elif k.endswith("norm.bias"):
            sd[k] = 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("running_mean"):
            sd[k] = 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shp, generator=g)
    return sd
