"""The reference of the mode-seeking regulariser (include/aclgan_hip.h: aclgan_modeseek / aclgan_ctx_set_modeseek) for the
tests: the definition as a torch function of (I, I', u, u'), its closed-form gradient seeds, and the term built onto the oracle's gen_update
graph from the oracle's public functions."""
import torch

from oracle import aclgan_oracle as O

EPS = 1e-5


def ms_terms(I, I2, u, u2):
    """per image: (dI_b, dz_b, ms_b, div_b).  I, I2: (B, ...) images; u, u2: (B, ...) noise rows (already scaled).  dz_b == 0 gives ms_b = div_b = 0."""
    B = I.shape[0]
    dI = (I - I2).abs().reshape(B, -1).mean(1)
    dz = (u - u2).abs().reshape(B, -1).mean(1)
    ok = dz > 0
    safe = torch.where(ok, dz, torch.ones_like(dz))
    ms = torch.where(ok, dz / (dI + EPS * safe), torch.zeros_like(dI))
    div = torch.where(ok, dI / safe, torch.zeros_like(dI))
    return dI, dz, ms, div


def ms_value(I, I2, u, u2):
    """(loss_gen_ms, div) of one direction: the means over the batch"""
    _, _, ms, div = ms_terms(I, I2, u, u2)
    return ms.mean(), div.mean()


def ms_seeds(I, I2, u, u2, lam, S=1.0):
    """the closed-form gradient seeds (dL/dI, dL/dI') of lam * loss_gen_ms, and the per-image coefficient k_b = S (lam / B) dz_b / (dI_b + eps dz_b)^2 / N"""
    B = I.shape[0]
    N = I[0].numel()
    dI, dz, _, _ = ms_terms(I, I2, u, u2)
    k = torch.where(dz > 0, S * (lam / B) * dz / (dI + EPS * dz) ** 2 / N, torch.zeros_like(dI))
    g = -k.reshape(B, *([1] * (I.dim() - 1))) * torch.sign(I - I2)
    return g, -g, k


def gen_losses_ms(nets, x_a, x_b, z, z_ms, hp):
    """oracle.gen_losses plus the mode-seeking pairs of both directions.  z_ms = (z_4, z_5), each (B, style_dim, 1, 1).
    Returns (total without the term, the 12 losses, fw, {'ms_B', 'div_B', 'ms_A', 'div_A'}): the objective is total + lam * (ms_B + ms_A)."""
    total, L, fw = O.gen_losses(nets, x_a, x_b, z, hp)
    g = hp["gen"]
    alpha = hp["alpha"]
    z4, z5 = z_ms

    def second(P, c, zz):
        d = O.decode(P, c, zz, g)
        if hp["focus_loss"] > 0:
            img, f = d.split(3, 1)
            return O.focus_translation(img, x_a, f)
        return d
    IB2 = second(nets["gen_AB"], fw["c_1"], z4)
    IA2 = second(nets["gen_BA"], fw["c_2"], alpha * z5)
    msB, divB = ms_value(fw["x_B_fake"], IB2, z[0], z4)
    msA, divA = ms_value(fw["x_A_fake"], IA2, alpha * z[1], alpha * z5)
    return total, L, fw, {"ms_B": msB, "div_B": divB, "ms_A": msA, "div_A": divA}
