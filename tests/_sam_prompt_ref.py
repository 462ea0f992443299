"""What the promptable-SAM tests share: the prompt cases of tests/golden/sam_prompts.npz (one definition for the generator and the
tests), the synthetic operands, and an fp64 NumPy restatement of the point / box encoding and of the mask downscaling
(prompt_encoder.py:78-114, 203-214, 231-238).  The restatement is pinned to the reference's own outputs by
tests/test_sam_prompt_cpu.py; the small-shape GPU tests then use it where the golden has no case."""
import numpy as np

IMG = 1024            # the padded input frame of the golden cases
GRID = 64
PHOTO = (750, 500)    # (H, W) of the photo of the coordinate-scaling and post-processing cases ...
PHOTO_INPUT = (1024, 683)  # ... and its resized size inside the padded square
CASES = ("a", "b", "c", "d", "e")


def _bf16(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def image_embedding():
    """the one synthetic image embedding of every case, fp32 [1,256,64,64] holding bf16 values"""
    from interactvlm_amd import synth

    return _bf16(synth.synth_normal("samprompt/image_emb", (1, 256, GRID, GRID), 1.0, 0))


def mask_inputs(B=2):
    """N(0, 5^2) logits with one constant 32x32 patch per prompt, fp32 [B,1,256,256]"""
    from interactvlm_amd import synth

    m = synth.synth_normal("samprompt/mask_input", (B, 1, 4 * GRID, 4 * GRID), 5.0, 0)
    for b in range(B):
        m[b, 0, 40 + 64 * b: 72 + 64 * b, 96: 128] = 7.5 - 15.0 * b
    return m


def case(name):
    """-> dict(points [B,N,2] | None, labels [B,N] | None, boxes [B,4] | None, mask_input [B,1,256,256] | None): coordinates in the
    padded 1024 x 1024 input frame, with non-integer values and the two corner pixels (0, 0) and (W - 1, H - 1)"""
    f, i = np.float32, np.int32
    if name == "a":  # one positive point (N = 2 with the pad)
        return dict(points=np.array([[[500.25, 375.5]]], f), labels=np.array([[1]], i), boxes=None, mask_input=None)
    if name == "b":  # two positive points and one negative
        return dict(points=np.array([[[0.0, 0.0], [1023.0, 1023.0], [300.75, 620.125]]], f), labels=np.array([[1, 1, 0]], i),
                    boxes=None, mask_input=None)
    if name == "c":  # box only
        return dict(points=None, labels=None, boxes=np.array([[100.5, 150.25, 700.0, 900.75]], f), mask_input=None)
    if name == "d":  # three prompts, points + box (no pad), different per prompt
        return dict(points=np.array([[[200.5, 300.0], [640.25, 512.75]], [[0.0, 0.0], [77.125, 901.5]], [[1023.0, 1023.0], [512.0, 512.0]]], f),
                    labels=np.array([[1, 0], [1, 1], [0, 1]], i),
                    boxes=np.array([[150.0, 250.5, 700.25, 600.0], [0.0, 0.0, 400.5, 1023.0], [480.75, 470.25, 1023.0, 1023.0]], f),
                    mask_input=None)
    if name == "e":  # two prompts, a point and a mask input
        return dict(points=np.array([[[256.5, 256.5]], [[700.0, 333.25]]], f), labels=np.array([[1], [1]], i), boxes=None,
                    mask_input=mask_inputs(2))
    raise KeyError(name)


def photo_coords():
    """(x, y) in the pixels of a 750 x 500 photo (PHOTO), for the coordinate-scaling check: [K,2] fp64"""
    return np.array([[0.0, 0.0], [499.0, 749.0], [123.25, 456.5], [250.0, 375.0], [499.5, 0.25]], np.float64)


# ---- weights ---------------------------------------------------------------------------------------------------------------------------
def prompt_weights(embed_dim=256):
    """the synthetic prompt-encoder tensors as the device path holds them: every parameter rounded to bf16, the Gaussian matrix not"""
    from interactvlm_amd import weights as Wt

    p = Wt.SAM_PREFIX + ".prompt_encoder"
    w = Wt.synth_weights(Wt.prompt_encoder_spec(embed_dim=embed_dim))
    out = {k[len(p) + 1:]: (v.numpy() if "gaussian" in k else _bf16(v.numpy())) for k, v in w.items()}
    return out


def point_table(pw):
    """[5, C]: negative point, positive point, box corner 0, box corner 1, not-a-point"""
    return np.concatenate([pw[f"point_embeddings.{i}.weight"] for i in range(4)] + [pw["not_a_point_embed.weight"]], 0)


def mask_down_weights(pw):
    """the ten tensors of mask_downscaling in the order ops.mask_downscale takes them"""
    return [pw["mask_downscaling." + n] for n in ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias", "4.weight",
                                                   "4.bias", "6.weight", "6.bias")]


# ---- fp64 restatement ------------------------------------------------------------------------------------------------------------------
def embed_rows_ref(coords, labels, gauss, table, size):
    """coords [R,2] (x, y), labels [R], gauss [2,F], table [5,2F], size (H, W) -> fp64 [R,2F]: [sin a | cos a] + table[label] with
    a = 2 pi ((2 (coord + 0.5) / (W, H) - 1) @ gauss); label -1 -> the not-a-point row alone; a label outside -1..3 -> NaN"""
    coords, gauss, table = (np.asarray(t, np.float64) for t in (coords, gauss, table))
    labels = np.asarray(labels)
    c = (coords + 0.5) / np.array([size[1], size[0]], np.float64)
    a = 2.0 * np.pi * ((2.0 * c - 1.0) @ gauss)
    out = np.concatenate([np.sin(a), np.cos(a)], -1)
    for r, lab in enumerate(labels):
        if lab == -1:
            out[r] = table[4]
        elif 0 <= lab <= 3:
            out[r] += table[lab]
        else:
            out[r] = np.nan
    return out


def sparse_ref(points, labels, boxes, gauss, table, size):
    """PromptEncoder.forward's sparse embeddings [B,N',2F] in fp64: the points, the pad point only when there is no box, the corners"""
    rows_c, rows_l = [], []
    B = (points if points is not None else boxes).shape[0]
    if points is not None:
        rows_c.append(np.asarray(points, np.float64))
        rows_l.append(np.asarray(labels, np.int64))
        if boxes is None:
            rows_c.append(np.zeros((B, 1, 2)))
            rows_l.append(-np.ones((B, 1), np.int64))
    if boxes is not None:
        rows_c.append(np.asarray(boxes, np.float64).reshape(B, 2, 2))
        rows_l.append(np.tile(np.array([[2, 3]], np.int64), (B, 1)))
    c, l = np.concatenate(rows_c, 1), np.concatenate(rows_l, 1)
    return embed_rows_ref(c.reshape(-1, 2), l.reshape(-1), gauss, table, size).reshape(B, l.shape[1], -1)


def _erf(x):
    from math import erf

    return np.vectorize(erf, otypes=[np.float64])(x)


def _gelu(x):
    return 0.5 * x * (1.0 + _erf(x / np.sqrt(2.0)))


def _ln_last(x, w, b, eps):
    u = x.mean(-1, keepdims=True)
    s = ((x - u) ** 2).mean(-1, keepdims=True)
    return (x - u) / np.sqrt(s + eps) * w + b


def mask_downscale_ref(mask, ws, eps=1e-6):
    """mask [B,4gh,4gw], ws = mask_down_weights -> fp64 [B, gh*gw, C] (channels last): conv k2s2 (1 -> 4) -> LayerNorm2d -> GELU ->
    conv k2s2 (4 -> 16) -> LayerNorm2d -> GELU -> conv 1x1 (16 -> C)"""
    w0, b0, g1, e1, w3, b3, g2, e2, w6, b6 = (np.asarray(t, np.float64) for t in ws)
    m = np.asarray(mask, np.float64)
    B, H, W = m.shape
    c1, c2 = b0.size, b3.size
    p = m.reshape(B, H // 2, 2, W // 2, 2)  # [B, y, ky, x, kx]
    h1 = np.einsum("bykxl,ckl->byxc", p, w0.reshape(c1, 2, 2)) + b0
    h1 = _gelu(_ln_last(h1, g1, e1, eps))
    p = h1.reshape(B, H // 4, 2, W // 4, 2, c1)  # [B, y, ky, x, kx, c]
    h2 = np.einsum("bykxlc,ockl->byxo", p, w3.reshape(c2, c1, 2, 2)) + b3
    h2 = _gelu(_ln_last(h2, g2, e2, eps))
    out = h2 @ w6.reshape(-1, c2).T + b6
    return out.reshape(B, (H // 4) * (W // 4), -1)

