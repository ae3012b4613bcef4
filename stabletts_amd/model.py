"""Drop-in replacement for the reference's ``models/model.py``: ``StableTTS`` and ``generate_path``
(``install(model=True)`` registers this module as ``models.model``, which ``train.py:18`` and ``api.py`` import).

``StableTTS`` keeps the reference constructor (models/model.py:31), its attributes (``n_vocab``, ``mel_channels``,
``fake_speaker``, ``fake_content``, ``cfg_dropout``) and its checkpoint keys, and is built from this package's own classes: the
native ``TextEncoder`` and ``CFMDecoder`` and the trainable ``MelStyleEncoder`` / ``DurationPredictor``.  Nothing of the
reference has to be importable.

``forward`` follows models/model.py:136-178 line by line: the cfg mask is drawn by the same ``torch.rand`` call at the same
point, the alignment search is ``alignment.monotonic_alignment`` and everything behind it -- ``logw_``, the duration loss,
``mu_y``, its cfg masking, the prior loss, and their gradients -- is ``alignment.align_and_losses``.  What is left to torch is the
masks from the lengths, the ``(B, gin)`` mixing of the speaker vector with ``fake_speaker`` and the random draws.
``synthesise`` follows :79-112 on ``alignment.length_regulate`` and the native decoder.  There is no CPU fallback.

Under DistributedDataParallel the class behaves as its submodules do: every parameter gradient is produced by an autograd
node, so the reducer's hooks fire; ``fake_content`` receives its gradient from ``align_and_losses``.
"""
import torch
import torch.nn as nn

from .alignment import align_and_losses, generate_path, length_regulate, monotonic_alignment  # noqa: F401  (generate_path: exported)
from .duration_predictor_train import DurationPredictor
from .flow_matching import CFMDecoder
from .reference_encoder_train import MelStyleEncoder
from .text_encoder import TextEncoder

__all__ = ["StableTTS", "generate_path"]


def sequence_mask(length, max_length=None):
    """utils/mask.py:4-8."""
    if max_length is None:
        max_length = length.max()
    x = torch.arange(max_length, dtype=length.dtype, device=length.device)
    return x.unsqueeze(0) < length.unsqueeze(1)


class StableTTS(nn.Module):
    return_attn = True          # forward's fourth value; train.py discards it, set False to return None instead

    def __init__(self, n_vocab, mel_channels, hidden_channels, filter_channels, n_heads, n_enc_layers, n_dec_layers, kernel_size,
                 p_dropout, gin_channels):
        super().__init__()
        self.n_vocab = n_vocab
        self.mel_channels = mel_channels

        self.encoder = TextEncoder(n_vocab, mel_channels, hidden_channels, filter_channels, n_heads, n_enc_layers, kernel_size,
                                   p_dropout, gin_channels)
        self.ref_encoder = MelStyleEncoder(mel_channels, style_vector_dim=gin_channels, style_kernel_size=5, dropout=0.25)
        self.dp = DurationPredictor(hidden_channels, filter_channels, kernel_size, 0.5, gin_channels)
        self.decoder = CFMDecoder(mel_channels, mel_channels, hidden_channels, mel_channels, filter_channels, n_heads, n_dec_layers,
                                  kernel_size, p_dropout, gin_channels)

        # uncondition input for cfg (models/model.py:42-44)
        self.fake_speaker = nn.Parameter(torch.zeros(1, gin_channels))
        self.fake_content = nn.Parameter(torch.zeros(1, mel_channels, 1))

        self.cfg_dropout = 0.2

    @torch.inference_mode()
    def synthesise(self, x, x_lengths, n_timesteps, temperature=1.0, y=None, length_scale=1.0, solver=None, cfg=1.0):
        """models/model.py:79-112: text ids (B, Tx), their lengths and a reference mel y (B, mel_channels, T) ->
        dict(encoder_outputs (B, mel_channels, Ty), decoder_outputs (B, mel_channels, Ty), attn (B, 1, Tx, Ty))."""
        c = self.ref_encoder(y, None)
        x, mu_x, x_mask = self.encoder(x, c, x_lengths)
        logw = self.dp(x, x_mask, c)

        lr = length_regulate(logw, x_mask, mu_x, length_scale)          # :83-95
        mu_y, y_mask = lr["mu_y"], lr["y_mask"]

        if cfg == 1.0:
            decoder_outputs = self.decoder(mu_y, y_mask, n_timesteps, temperature, c, solver)
        else:
            cfg_kwargs = {'fake_speaker': self.fake_speaker, 'fake_content': self.fake_content, 'cfg_strength': cfg}
            decoder_outputs = self.decoder(mu_y, y_mask, n_timesteps, temperature, c, solver, cfg_kwargs)

        return {"encoder_outputs": mu_y, "decoder_outputs": decoder_outputs, "attn": lr["attn"]}

    def forward(self, x, x_lengths, y, y_lengths, z, z_lengths):
        """models/model.py:136-178: (dur_loss, diff_loss, prior_loss, attn (B, Tx, Ty) or None without return_attn)."""
        y_mask = sequence_mask(y_lengths, y.size(2)).unsqueeze(1).to(y.dtype)
        z_mask = sequence_mask(z_lengths, z.size(2)).unsqueeze(1).to(z.dtype)
        cfg_mask = torch.rand(y.size(0), 1, device=y.device) > self.cfg_dropout

        # global speaker embedding (:141); (B, gin), stays in torch
        c = self.ref_encoder(z, z_mask) * cfg_mask + ~cfg_mask * self.fake_speaker.repeat(z.size(0), 1)

        x, mu_x, x_mask = self.encoder(x, c, x_lengths)
        logw = self.dp(x, x_mask, c)

        mas = monotonic_alignment(mu_x, x_mask, y, y_mask)             # :148-158, no gradient
        out = align_and_losses(mu_x, x_mask, logw, x_lengths, y, y_mask, mas["durations"], keep=cfg_mask,
                               fake_content=self.fake_content)        # :162-172, :175-176
        diff_loss, _ = self.decoder.compute_loss(y, y_mask, out["mu_y_masked"], c)

        attn = mas["attn"].squeeze(1).transpose(1, 2) if self.return_attn else None      # :166, the search's own path
        return out["dur_loss"], diff_loss, out["prior_loss"], attn
