"""2x-AnimeSharpV4 (RCAN) upscaler on libmtx_hip — the model object `ModelManager.load_upscale*`
returns (reference core/ml/model_manager.py:617-700 builds it with spandrel; the operator calls
`model(tensor[1,3,H,W] fp32 0..1)`, reference core/image/image_utils.py:369-374).

Architecture hyper-parameters come from the checkpoint's tensor shapes (as an auto-detecting
loader does); weights are repacked ONCE at load into the kernels' layout:
  conv weights [Cout][3x3 taps][Cin] f16 (Cin padded to 8), the pixel-shuffle convs with their
  output channels permuted to (dy, dx, c) so PixelShuffle(2) is pure store addressing.
A forward pass is one native `mtx_plan_run` of a static graph per input shape:

  img(NCHW f32 -> NHWC f16, *rgb_range, -mean, pixel-unshuffle) -> head conv
  per RCAB: conv+ReLU -> conv (+ per-tile channel sums fused) -> squeeze/excite MLP -> scale+skip
  group/long skips fused into the conv epilogues -> upsampler conv(s) with fused pixel shuffle
  -> tail conv -> img(NHWC -> NCHW f32, /rgb_range, +mean)

fp16 storage / fp32 MFMA accumulation: the trunk of a 400-conv residual network loses ~1e-3
relative accuracy per rounding with bf16 (8-bit mantissa), which does not hold PSNR >= 40 dB;
fp16's 11-bit mantissa does, and activations are O(rgb_range) so its range suffices
(saturating converts guard outliers).
"""
import math
import re
import threading

import torch

from ...hip import abi
from ...hip.lib import get_library
from ...hip.plan import PlanBuilder, PlanCache
from ...utils.exceptions import ModelError
from . import packing


def derive_rcan_hparams(sd: dict) -> dict:
    """Architecture from tensor shapes (state-dict key layout of the EDSR-style RCAN)."""
    try:
        n_feats, in_ch = sd["head.0.weight"].shape[:2]
        gb = {}
        for k in sd:
            m = re.match(r"body\.(\d+)\.body\.(\d+)\.", k)
            if m:
                g, b = int(m.group(1)), int(m.group(2))
                gb[g] = max(gb.get(g, -1), b)
        n_resgroups = len(gb)
        n_resblocks = gb[0]
        cr = sd["body.0.body.0.body.3.conv_du.0.weight"].shape[0]
        up_keys = sorted(int(m.group(1)) for k in sd for m in [re.match(r"tail\.0\.(\d+)\.weight$", k)] if m)
        n_colors = sd["tail.1.weight"].shape[0]
    except KeyError as e:
        raise ModelError(f"not an RCAN checkpoint (missing {e})") from e
    ups = []
    for u in up_keys:
        ratio = sd[f"tail.0.{u}.weight"].shape[0] // n_feats
        if ratio != 4:
            raise ModelError(f"RCAN upsampler stage tail.0.{u} has factor^2={ratio}; only PixelShuffle(2) stages are built")
        ups.append(u)
    if n_colors != 3:
        raise ModelError("RCAN: only 3-colour models are supported")
    unshuffle = int(round(math.sqrt(in_ch // n_colors)))
    if unshuffle not in (1, 2) or unshuffle * unshuffle * n_colors != in_ch:
        raise ModelError(f"RCAN: unsupported head input channels {in_ch}")
    if n_feats % 8:
        raise ModelError("RCAN: n_feats must be a multiple of 8")
    return dict(n_feats=int(n_feats), n_resgroups=n_resgroups, n_resblocks=n_resblocks, cr=int(cr),
                up_keys=ups, unshuffle=unshuffle, scale=(2 ** len(ups)) // unshuffle,
                mean_shift=("sub_mean.weight" in sd))


def shuffle_order(t: torch.Tensor) -> torch.Tensor:
    """output channels (dim 0) of a conv that feeds PixelShuffle(2): torch reads channel c * 4 + dy * 2 + dx, the store wants (dy * 2 + dx) * C + c"""
    return t.view(t.shape[0] // 4, 4, *t.shape[1:]).transpose(0, 1).reshape(t.shape)


def read_safetensors_header(path) -> dict:
    """{tensor name: shape} from a .safetensors file's JSON header alone (8-byte little-endian length, then the JSON): the
    hyper-parameters of an upscaler checkpoint can be told without reading 20-60 MB of weights"""
    import json
    import struct
    with open(path, "rb") as f:
        (n,) = struct.unpack("<Q", f.read(8))
        if n <= 0 or n > (100 << 20):
            raise ModelError(f"{path}: not a safetensors file (header length {n})")
        head = json.loads(f.read(n).decode("utf-8"))
    return {k: tuple(v["shape"]) for k, v in head.items() if k != "__metadata__"}


def rcan_hparams_from_header(path) -> dict:
    """`derive_rcan_hparams` on the shapes in a checkpoint's header (2x-AnimeSharpV4_RCAN / _Fast_RCAN_PU, reference
    core/ml/model_manager.py:617-700): n_feats, n_resgroups, n_resblocks, reduction, scale and the pixel-unshuffle factor of the
    "PU" variants come from the tensor shapes, nothing is assumed"""
    shapes = read_safetensors_header(path)
    return derive_rcan_hparams({k: torch.empty(s, device="meta") for k, s in shapes.items()})


class RCANUpscaler:
    """Callable like the spandrel model descriptor: `model(tensor[N,3,H,W] f32) -> [N,3,sH,sW] f32`.
    Thread-safe (up to 20 reference worker threads share one instance)."""

    def __init__(self, state_dict: dict, device="cuda", rgb_range: float = 255.0, lib=None, graph: bool = True, pool_before_conv: bool = True,
                 ca_split: bool = True):
        """pool_before_conv: the channel attention of an RCAB is computed from the sums of conv1's output before conv2 runs, and conv2
        writes x + s * conv2(t) itself (3 launches, 5 activation passes per RCAB); False: the 4-launch / 7-pass form (conv2 -> pool ->
        attention -> scale-and-add pass).  Needs n_feats <= 64 in multiples of 8 (mtx_ca_args.t).
        ca_split: the attention launch between the two convs runs on MTX_CA_SPLIT workgroups per image (mtx_ca_args.scratch); False: one
        workgroup per image (round 2's form, kept for same-box A/Bs)"""
        self.lib = lib if lib is not None else get_library()
        self.device = torch.device(device)
        self.hp = derive_rcan_hparams(state_dict)
        self.scale = self.hp["scale"]
        self.rgb_range = float(rgb_range)
        self.dtype = abi.F16
        self._tdt = torch.float16
        self._graph = graph and not self.lib.is_simulator
        self._lock = threading.RLock()
        self._plans = PlanCache(8)          # pages of one size reuse their plan
        self._buckets = PlanCache(32)       # bubble crops (any size up to BUCKET_MAX) share masked bucket plans
        self._big_buckets = PlanCache(6)    # ... and the few larger ones (a 1024 x 1024 canvas pins ~2 GB of activations)
        self._pack(state_dict)
        self.pool_before_conv = pool_before_conv and self.hp["n_feats"] <= 64 and self.hp["n_feats"] % 8 == 0
        self.ca_split = ca_split

    # ---- weights ----------------------------------------------------------------------------
    def _pack(self, sd):
        dev, dt, hp = self.device, self._tdt, self.hp
        f = lambda t: t.detach().float().cpu()
        W = {}

        def conv(name, key, shuffle=False, cout_pad=0):
            w = f(sd[key + ".weight"])
            b = f(sd[key + ".bias"]) if key + ".bias" in sd else torch.zeros(w.shape[0])
            if shuffle:
                w, b = shuffle_order(w), shuffle_order(b)
            W[name] = (packing.on_device(packing.conv_taps(w, cout_pad=cout_pad), dev, dt), packing.on_device(packing.padded_bias(b, cout_pad), dev))

        conv("head", "head.0")
        for g in range(hp["n_resgroups"]):
            for b in range(hp["n_resblocks"]):
                p = f"body.{g}.body.{b}.body"
                conv(f"g{g}b{b}c1", p + ".0")
                conv(f"g{g}b{b}c2", p + ".2")
                W[f"g{g}b{b}ca"] = tuple(packing.on_device(f(sd[p + k]).reshape(s), dev) for k, s in (
                    (".3.conv_du.0.weight", (hp["cr"], hp["n_feats"])), (".3.conv_du.0.bias", (hp["cr"],)),
                    (".3.conv_du.2.weight", (hp["n_feats"], hp["cr"])), (".3.conv_du.2.bias", (hp["n_feats"],))))
            conv(f"g{g}tail", f"body.{g}.body.{hp['n_resblocks']}")
        conv("body_tail", f"body.{hp['n_resgroups']}")
        for i, u in enumerate(hp["up_keys"]):
            conv(f"up{i}", f"tail.0.{u}", shuffle=True)
        conv("tail", "tail.1", cout_pad=8)
        self.W = W
        self.mean = [0.0, 0.0, 0.0]
        if hp["mean_shift"]:
            wsub, wadd = f(sd["sub_mean.weight"]).view(3, 3), f(sd["add_mean.weight"]).view(3, 3)
            if not (torch.allclose(wsub, torch.eye(3)) and torch.allclose(wadd, torch.eye(3))):
                raise ModelError("RCAN: MeanShift with non-identity weight is not supported")
            self.sub_bias = [float(v) for v in f(sd["sub_mean.bias"])]
            self.add_bias = [float(v) for v in f(sd["add_mean.bias"])]
        else:
            self.sub_bias = [0.0, 0.0, 0.0]
            self.add_bias = [0.0, 0.0, 0.0]

    # ---- graph ------------------------------------------------------------------------------
    def _build(self, n, h, w, bucket: bool = False):
        """bucket: the plan is built on an h x w CANVAS and every layer masks its output to the image size it finds in `plan.valid`
        (include/mtx_hip.h `valid_hw`): one plan serves every image that fits, with the zero padding of its true size"""
        hp, W = self.hp, self.W
        u = hp["unshuffle"]
        if h % u or w % u:
            raise ModelError(f"RCAN(PU): plans are built on sizes divisible by {u} (callers pad: see _padded)")
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        C_ = hp["n_feats"]
        x_in = pb.buf((n, 3, h, w), torch.float32)
        cin_pad = (3 * u * u + 7) // 8 * 8
        hh, ww = h // u, w // u
        a0 = pb.act(n, hh, ww, cin_pad)
        valid_src = pb.buf((2,), torch.int32, zero=True) if bucket else None       # image size in source pixels
        valid = pb.buf((2,), torch.int32, zero=True) if bucket else None           # ... on the trunk's grid (after the pixel unshuffle)
        valid_up = [pb.buf((2,), torch.int32, zero=True) for _ in hp["up_keys"]] if bucket else []       # ... after each 2x stage
        inv_hw_dev = pb.buf((1,), torch.float32, zero=True) if bucket else None
        vk = dict(valid_hw=valid) if bucket else {}
        pb.image_convert(abi.IMG_NCHW_F32_TO_NHWC, x_in, a0.t, n, h, w, cin_pad, unshuffle=u,
                         mul=self.rgb_range, add=self.sub_bias, label="to_nhwc", valid_hw=valid_src)
        head = pb.conv2d(a0, *W["head"], cout=C_, label="head", **vk)
        tiles = pb.conv_tiles(head)
        chan_sum = pb.buf((n, tiles, C_), torch.float32)
        s_buf = pb.buf((n, C_), torch.float32)
        t1 = pb.act(n, hh, ww, C_)
        t2 = pb.act(n, hh, ww, C_)
        ping = [pb.act(n, hh, ww, C_) for _ in range(3)]
        cur = head
        inv_hw = 1.0 / float(hh * ww)
        pi = 0

        def next_buf(avoid):
            nonlocal pi
            for _ in range(3):
                cand = ping[pi % 3]
                pi += 1
                if all(cand.t is not a.t for a in avoid):
                    return cand
            raise AssertionError

        for g in range(hp["n_resgroups"]):
            gin = cur
            for b in range(hp["n_resblocks"]):
                w1, b1, w2, b2 = W[f"g{g}b{b}ca"]
                nxt = next_buf([cur, gin, head])
                if self.pool_before_conv:
                    # RCAB in three launches and five activation passes (was four and seven): conv1 also sums its output t; the channel
                    # attention of conv2(t) follows from those sums by linearity (mtx_ca_args.t) BEFORE conv2 runs; conv2 then writes
                    # x + s * (conv2(t) + b) itself, in fp32 with one rounding — no separate scale-and-add pass over the activations
                    pb.conv2d(cur, *W[f"g{g}b{b}c1"], cout=C_, act=abi.ACT_RELU, out=t1, chan_sum=chan_sum, label=f"g{g}b{b}.conv1", **vk)
                    cw, cb = W[f"g{g}b{b}c2"]
                    pb.channel_attention(chan_sum, w1, b1, w2, b2, s_buf, n, tiles, C_, hp["cr"], inv_hw, label=f"g{g}b{b}.ca", inv_hw_dev=inv_hw_dev,
                                         before_conv=(t1, cw, cb), valid_hw=valid, split=self.ca_split)
                    pb.conv2d(t1, cw, cb, cout=C_, out=nxt, res=cur, out_scale=s_buf, label=f"g{g}b{b}.conv2", **vk)
                else:
                    pb.conv2d(cur, *W[f"g{g}b{b}c1"], cout=C_, act=abi.ACT_RELU, out=t1, label=f"g{g}b{b}.conv1", **vk)
                    pb.conv2d(t1, *W[f"g{g}b{b}c2"], cout=C_, out=t2, chan_sum=chan_sum, label=f"g{g}b{b}.conv2", **vk)
                    pb.channel_attention(chan_sum, w1, b1, w2, b2, s_buf, n, tiles, C_, hp["cr"], inv_hw, label=f"g{g}b{b}.ca", inv_hw_dev=inv_hw_dev)
                    pb.ew(abi.EW_SCALE_RES, t2, b=cur, s=s_buf, out=nxt, lds=C_, label=f"g{g}b{b}.scale_skip")
                cur = nxt
            nxt = next_buf([cur, gin, head])
            pb.conv2d(cur, *W[f"g{g}tail"], cout=C_, res=gin, out=nxt, label=f"g{g}.tail", **vk)
            cur = nxt
        body = pb.conv2d(cur, *W["body_tail"], cout=C_, res=head, out=t1, label="body_tail", **vk)
        up = body
        for i in range(len(hp["up_keys"])):       # the mask of a pixel-shuffle conv is taken on its INPUT grid
            up = pb.conv2d(up, *W[f"up{i}"], cout=4 * C_, pixel_shuffle=2, label=f"up{i}", valid_hw=(valid if i == 0 else valid_up[i - 1]) if bucket else None)
        y8 = pb.conv2d(up, *W["tail"], cout=8, label="tail", valid_hw=valid_up[-1] if (bucket and valid_up) else (valid if bucket else None))
        oh, ow = up.h, up.w
        y_out = pb.buf((n, 3, oh, ow), torch.float32)
        inv = 1.0 / self.rgb_range
        pb.image_convert(abi.IMG_NHWC_TO_NCHW_F32, y8.t, y_out, n, oh, ow, 8, mul=inv,
                         add=[v * inv for v in self.add_bias], label="to_nchw")
        y_u8 = pb.buf((n, oh, ow, 3), torch.uint8)
        # tensor_to_image fused: clamp(0,1)*255 truncated to uint8 HWC (image_utils.py:361-366)
        pb.image_convert(abi.IMG_NHWC_TO_HWC_U8, y8.t, y_u8, n, oh, ow, 8, mul=inv,
                         add=[v * inv for v in self.add_bias], label="to_u8")
        plan = pb.build()
        plan.x_in, plan.y_out, plan.y8, plan.y_u8 = x_in, y_out, y8, y_u8
        plan.out_scale = (inv, [v * inv for v in self.add_bias])
        plan.valid_bufs = (valid_src, valid, valid_up, inv_hw_dev) if bucket else None
        return plan

    BUCKET = 64            # bucket plans: canvas sides are multiples of this ...
    BUCKET_MAX = 512       # ... up to this: a crop below the minimum side takes up to two passes, the second on <= 2 x its size
    BIG_BUCKET = 128       # sides between BUCKET_MAX and BIG_BUCKET_MAX (large bubble crops, second passes): coarser steps, a small cache of
    BIG_BUCKET_MAX = 1024  # their own — exact-size plans for them rebuilt and re-captured a hipGraph for almost every crop.
                           # Larger images — pages — get a plan of their own size.

    def _bucket_plan(self, h, w):
        """(plan, canvas_h, canvas_w) for an image of h x w source pixels (already a multiple of the unshuffle factor), or None"""
        if max(h, w) > self.BIG_BUCKET_MAX:
            return None
        big = max(h, w) > self.BUCKET_MAX
        step = self.BIG_BUCKET if big else self.BUCKET
        bh, bw = (h + step - 1) // step * step, (w + step - 1) // step * step
        key = ("bucket", bh, bw)
        cache = self._big_buckets if big else self._buckets
        with self._lock:
            if key not in cache:
                cache[key] = self._build(1, bh, bw, bucket=True)
            plan = cache[key]
        u = self.hp["unshuffle"]
        vs, v, vup, inv = plan.valid_bufs
        vs.copy_(torch.tensor([h, w], dtype=torch.int32))
        v.copy_(torch.tensor([h // u, w // u], dtype=torch.int32))
        for i, t in enumerate(vup):
            t.copy_(torch.tensor([(h // u) << (i + 1), (w // u) << (i + 1)], dtype=torch.int32))
        inv.fill_(1.0 / float((h // u) * (w // u)))
        return plan, bh, bw

    def plan_for(self, n, h, w):
        u = self.hp["unshuffle"]
        key = (n, h + (-h) % u, w + (-w) % u)
        with self._lock:
            if key not in self._plans:
                self._plans[key] = self._build(*key)
            return self._plans[key]

    def _padded(self, x: torch.Tensor):
        """[N,3,H,W] on the device, H and W brought up to multiples of the pixel-unshuffle factor by reflecting the last rows /
        columns (the pixel-unshuffle variants of the upstream architecture pad the same way and crop the result): pages and bubble
        crops come in any size (reference image_utils.py:369-374 calls the model on whatever it has)"""
        u = self.hp["unshuffle"]
        h, w = x.shape[-2:]
        ph, pw = (-h) % u, (-w) % u
        if ph or pw:
            mode = "reflect" if (h > ph and w > pw) else "replicate"
            x = torch.nn.functional.pad(x, (0, pw, 0, ph), mode=mode)
        return x, h, w

    # ---- the spandrel-model call shape -----------------------------------------------------------
    @torch.no_grad()
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4 or x.shape[1] != 3:
            raise ModelError(f"RCAN expects [N,3,H,W], got {tuple(x.shape)}")
        x, h, w = self._padded(x.to(device=self.device, dtype=torch.float32))
        n = x.shape[0]
        with self._lock:
            bp = self._bucket_plan(x.shape[2], x.shape[3]) if n == 1 else None
            if bp is not None:            # small image (bubble crop): masked run on a shared canvas
                plan, bh, bw = bp
                plan.x_in[:, :, : x.shape[2], : x.shape[3]].copy_(x)
                plan.run(graph=self._graph)
                s = plan.y_out.shape[2] // bh
                return plan.y_out[:, :, : h * s, : w * s].clone()
            plan = self.plan_for(n, x.shape[2], x.shape[3])
            plan.x_in.copy_(x)
            plan.run(graph=self._graph)
            s = plan.y_out.shape[2] // x.shape[2]
            return plan.y_out[:, :, : h * s, : w * s].clone()

    @torch.no_grad()
    def upscale_u8(self, page_u8: torch.Tensor) -> torch.Tensor:
        """[H,W,3] uint8 page (device or host) -> [sH,sW,3] uint8 on the device: image_to_tensor,
        model and tensor_to_image of the reference in one native plan run."""
        x = page_u8.to(self.device).permute(2, 0, 1).unsqueeze(0).to(torch.float32) / 255.0
        x, h, w = self._padded(x)
        with self._lock:
            bp = self._bucket_plan(x.shape[2], x.shape[3])
            if bp is not None:
                plan, bh, bw = bp
                plan.x_in[:, :, : x.shape[2], : x.shape[3]].copy_(x)
                plan.run(graph=self._graph)
                s = plan.y_u8.shape[1] // bh
                return plan.y_u8[0, : h * s, : w * s].clone()
            plan = self.plan_for(1, x.shape[2], x.shape[3])
            plan.x_in.copy_(x)
            plan.run(graph=self._graph)
            s = plan.y_u8.shape[1] // x.shape[2]
            return plan.y_u8[0, : h * s, : w * s].clone()

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    # FLOPs / algorithmic bytes of one forward, printed next to roofline numbers
    def work(self, h, w):
        hp = self.hp
        u = hp["unshuffle"]
        px = (h // u) * (w // u)
        C_ = hp["n_feats"]
        conv = 2 * 9 * C_ * C_ * px
        n_body = hp["n_resgroups"] * (2 * hp["n_resblocks"] + 1) + 1
        flops = 2 * 9 * (3 * u * u) * C_ * px + n_body * conv
        p = px
        for _ in hp["up_keys"]:
            flops += 2 * 9 * C_ * 4 * C_ * p
            p *= 4
        flops += 2 * 9 * C_ * 3 * p
        return dict(flops=flops, conv64_flops=conv, conv64_bytes=2 * C_ * px * 2 + 9 * C_ * C_ * 2, n_conv64=n_body)
