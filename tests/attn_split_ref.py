"""The arithmetic of the split-key decode attention (pcy_attn_decode_split), restated in torch on the CPU with its rounding
points spelled out, plus the two yardsticks it is held against: the eager bf16 formulas of the reference and float64 softmax attention on the
same bf16 inputs.  No GPU, no library."""
import torch
import torch.nn.functional as F

BF = torch.bfloat16
BF16_MIN = torch.finfo(BF).min


def scores(q_roped, K, scale, mask):
    """s_j = bf16(bf16(q.k) * scale), a masked s_j = the bf16 minimum.  q_roped [B,H,1,dh], K [B,H,n,dh] bf16; mask [B,n] (non-zero = kept) or
    None -> [B,H,n] bf16"""
    s = (torch.matmul(q_roped, K.transpose(2, 3)) * float(scale))[:, :, 0]       # (the product in fp32, rounded once)
    if mask is not None:
        s = s.masked_fill((mask == 0)[:, None, :], BF16_MIN)
    return s


def split_reference(q_roped, K, V, scale, mask, chunk_keys, prefix_T):
    """q_roped [B,H,1,dh], K / V [B,H,n,dh] bf16 over the logical slots [0, n) with the new token last (kv heads already repeated); mask [B,n]
    or None; the prefix slots [0, prefix_T) cut into chunks of chunk_keys keys, the slots [prefix_T, n) the last chunk -> o [B, H*dh] bf16.
    Per chunk: m_c = max s, e = exp(s - m_c) in fp32, l_c = sum e in fp32, p = bf16(e), o_c = sum p * v in fp32.  Combine: m = max m_c,
    w_c = exp(m_c - m), o = bf16((sum w_c o_c) / (sum w_c l_c)), both sums in chunk order, rounded once."""
    B, H, n, dh = K.shape
    assert chunk_keys > 0 and 0 < prefix_T < n
    s = scores(q_roped, K, scale, mask).float()
    cuts = list(range(0, prefix_T, chunk_keys)) + [prefix_T, n]
    ms, ls, os_ = [], [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sc = s[:, :, lo:hi]
        m_c = sc.max(-1).values
        e = torch.exp(sc - m_c[..., None])
        p = e.to(BF).float()
        ms.append(m_c)
        ls.append(e.sum(-1))
        os_.append(torch.matmul(p[:, :, None, :], V[:, :, lo:hi].float())[:, :, 0])
    m = torch.stack(ms).max(0).values
    num, den = torch.zeros(B, H, dh), torch.zeros(B, H)
    for m_c, l_c, o_c in zip(ms, ls, os_):
        w = torch.exp(m_c - m)
        num = num + w[..., None] * o_c
        den = den + w * l_c
    return (num / den[..., None]).to(BF).reshape(B, H * dh)


def eager_reference(q_roped, K, V, scale, mask):
    """the reference's bf16 formulas: p = bf16(softmax_fp32(s)) under the global (m, l), o = bf16(p . V)"""
    s = scores(q_roped, K, scale, mask)
    p = F.softmax(s[:, :, None, :], dim=-1, dtype=torch.float32).to(BF)
    B, H, n, dh = K.shape
    return torch.matmul(p, V)[:, :, 0].reshape(B, H * dh)


def truth64(q_roped, K, V, scale, mask):
    """float64 softmax attention on the same bf16 inputs (masked keys excluded exactly)"""
    s = torch.matmul(q_roped.double(), K.double().transpose(2, 3))[:, :, 0] * float(scale)
    if mask is not None:
        s = s.masked_fill((mask == 0)[:, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    B, H, n, dh = K.shape
    return torch.matmul(p[:, :, None, :], V.double())[:, :, 0].reshape(B, H * dh)


def rel64(a, truth):
    return float((a.double() - truth).norm() / truth.norm())
