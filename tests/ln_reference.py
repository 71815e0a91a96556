"""The fp64 LayerNorm reference and the element-wise bound of an fp32 evaluation of it, shared by the op tests of the image front
end (test_gpu_frontend_ops.py: ln_pre, ln_post) and of the text pass (test_gpu_text_pass_ops.py: score_embed_ln_kernel)."""
import torch

U = 2.0 ** -24           # fp32 unit roundoff


def ln_ref_and_bound(v, gamma, beta, eps, add=None):
    """fp64 LayerNorm of the rows v (+ add) and the bound of the kernels' fp32 evaluation, element by element.  With V = max |v|
    of the row, d = v - mean, s = sqrt(var + eps), u = 2^-24:
      v itself (ln_pre: src + pos; the text embedding: word + position) rounds once: u V.  The mean is a sum of D <= 1024 terms
      in at most 40 sequential roundings (<= 32 per lane + the 5 or 6 shuffle levels + the division) of partial sums <= D V / D:
      40 u V, + the u V of its terms.  (score_embed_ln_kernel: 3 adds per lane, 6 shuffle levels, 3 adds across the waves and
      the division, 13 roundings -- inside the 40.)
      d: |dd| <= 42 u V + u |d|.
      var: each d^2 moves by 2 |d| dd, the sum rounds 42 times: relative 84 u V / s + 44 u; rstd = rsqrt(var + eps) half of that
      + 3 u (the add and a 2-ulp rsqrtf): 42 u V / s + 25 u.
      y = d rstd gamma + beta (+ add): |gamma| / s * dd + |d / s gamma| (42 u V / s + 25 u + 4 u) + 2 u (|y| + |add|)."""
    v, g, b = v.double(), gamma.double(), beta.double()
    mean = v.mean(-1, keepdim=True)
    d = v - mean
    s = torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    yhat = d / s * g
    y = yhat + b
    a = torch.zeros_like(y) if add is None else add.double().expand_as(y)
    y = y + a
    V = v.abs().amax(-1, keepdim=True)
    bound = g.abs() / s * (42 * U * V + U * d.abs()) + yhat.abs() * (42 * U * V / s + 29 * U) + 2 * U * (y.abs() + a.abs())
    return y, bound
