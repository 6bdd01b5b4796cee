"""The VAE's decoder alone, restated with torch.nn.functional over the oracle's parameter dict (eval-mode BatchNorm): what
melo_gan_amd.ae.edit decodes is a latent that no encoder has just produced, and the oracle's vae_fwd only decodes its own z.
tests/test_latent_edit_cpu.py pins this file to O.vae_fwd(..., train=False): fed the z the oracle returns, it gives the oracle's
recon exactly."""
import torch
import torch.nn.functional as F

BN_EPS = 1e-5


def vae_decode(P, Bf, z, max_notes: int):
    """z (B, LATENT_DIM) -> recon (B, max_notes, 4): decoder.pre (2x Linear + ReLU) -> (B, 128, red) -> 3x ConvTranspose1d
    (k 5, s 2, p 2, output_padding 1; BatchNorm + ReLU after the first two, tanh after the last) -> cut or zero-padded to
    max_notes rows."""
    y = F.relu(F.linear(z, P["decoder.pre.0.weight"], P["decoder.pre.0.bias"]))
    y = F.relu(F.linear(y, P["decoder.pre.2.weight"], P["decoder.pre.2.bias"]))
    y = y.view(y.shape[0], 128, -1)
    for i in (0, 3):
        y = F.conv_transpose1d(y, P[f"decoder.deconv.{i}.weight"], P[f"decoder.deconv.{i}.bias"], stride=2, padding=2,
                               output_padding=1)
        nm = f"decoder.deconv.{i + 1}"
        y = F.relu(F.batch_norm(y, Bf[nm + ".running_mean"], Bf[nm + ".running_var"], P[nm + ".weight"], P[nm + ".bias"], False, 0.1,
                                BN_EPS))
    y = torch.tanh(F.conv_transpose1d(y, P["decoder.deconv.6.weight"], P["decoder.deconv.6.bias"], stride=2, padding=2,
                                      output_padding=1))
    out = y.permute(0, 2, 1)
    if out.shape[1] > max_notes:
        out = out[:, :max_notes]
    elif out.shape[1] < max_notes:
        out = torch.cat([out, out.new_zeros(out.shape[0], max_notes - out.shape[1], out.shape[2])], dim=1)
    return out.contiguous()
