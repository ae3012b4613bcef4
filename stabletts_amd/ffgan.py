"""Drop-in for the reference's FireflyGAN vocoder, the default of ``api.py`` (``vocoder_name='ffgan'``, api.py:19-24,39):
``FireflyGANBaseWrapper(model_path)(mel) -> audio`` (vocoders/ffgan/model.py:32-57).

Same module tree as the reference (``backbone.downsample_layers.<i>.<j>``, ``backbone.stages.<i>.<j>.{dwconv,norm,pwconv1,
pwconv2,gamma}``, ``backbone.norm``, ``head.conv_pre``, ``head.ups.<i>``, ``head.resblocks.<i>.blocks.<b>.convs{1,2}.<p>``,
``head.conv_post``, the weight-normed convs as ``parametrizations.weight.original0`` / ``original1``), so the released
``firefly-gan-base-generator.ckpt`` loads with ``load_state_dict(strict=True)``.  The modules hold parameters only: the forward
pass runs in libstabletts_hip.so (st_ffgan_forward, st_ffgan_forward_ragged); there is no PyTorch fallback.  Inference only, like the reference.

The reference's ``remove_parametrizations`` helpers (head.py:110-114,251-256) raise TypeError and are not mirrored: the
engine folds the weight norm itself when it packs the weights.
"""
from math import prod

import torch
import torch.nn as nn
from torch.nn.utils.parametrizations import weight_norm

from . import _lib
from ._native_module import NativeModule, host_lengths
from .estimator import _ParamsOnly

config_dict = {                 # vocoders/ffgan/model.py:7-29
    "backbone": {
        "input_channels": 128,
        "depths": [3, 3, 9, 3],
        "dims": [128, 256, 384, 512],
        "drop_path_rate": 0.2,
        "kernel_size": 7,
    },
    "head": {
        "hop_length": 512,
        "upsample_rates": [8, 8, 2, 2, 2],
        "upsample_kernel_sizes": [16, 16, 4, 4, 4],
        "resblock_kernel_sizes": [3, 7, 11],
        "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]],
        "num_mels": 512,        # the output width of the backbone
        "upsample_initial_channel": 512,
        "use_template": False,
        "pre_conv_kernel_size": 13,
        "post_conv_kernel_size": 13,
    },
}


class LayerNorm(_ParamsOnly):
    """backbone.py:47-62.  Time-major, channels_first and channels_last are the same per-frame operation."""
    def __init__(self, normalized_shape, eps=1e-6, data_format="channels_last"):
        super().__init__()
        if data_format not in ("channels_last", "channels_first"):
            raise NotImplementedError
        if eps != 1e-6:
            raise NotImplementedError("native LayerNorm is built for eps = 1e-6 (the reference's only value)")
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps, self.data_format = eps, data_format


class ConvNeXtBlock(_ParamsOnly):
    """backbone.py:93-122 (parameters only; DropPath has none and is the identity in eval)."""
    def __init__(self, dim, drop_path=0.0, layer_scale_init_value=1e-6, mlp_ratio=4.0, kernel_size=7, dilation=1):
        super().__init__()
        if mlp_ratio != 4.0 or dilation != 1:
            raise NotImplementedError("native ConvNeXt block is built for mlp_ratio = 4, dilation = 1")
        if not layer_scale_init_value > 0:
            raise NotImplementedError("native ConvNeXt block is built with the layer scale (gamma)")
        self.dwconv = nn.Conv1d(dim, dim, kernel_size=kernel_size, padding=(kernel_size - 1) // 2, groups=dim)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones(dim), requires_grad=True)


class ConvNeXtEncoder(_ParamsOnly):
    """backbone.py:146-204."""
    def __init__(self, input_channels=3, depths=(3, 3, 9, 3), dims=(96, 192, 384, 768), drop_path_rate=0.0,
                 layer_scale_init_value=1e-6, kernel_size=7):
        super().__init__()          # drop_path_rate: DropPath holds no parameters and is the identity in eval
        assert len(depths) == len(dims)
        self.downsample_layers = nn.ModuleList()
        self.downsample_layers.append(nn.Sequential(
            nn.Conv1d(input_channels, dims[0], kernel_size=kernel_size, padding=kernel_size // 2),
            LayerNorm(dims[0], eps=1e-6, data_format="channels_first")))
        for i in range(len(depths) - 1):
            self.downsample_layers.append(nn.Sequential(LayerNorm(dims[i], eps=1e-6, data_format="channels_first"),
                                                        nn.Conv1d(dims[i], dims[i + 1], kernel_size=1)))
        self.stages = nn.ModuleList(
            nn.Sequential(*[ConvNeXtBlock(dim=dims[i], layer_scale_init_value=layer_scale_init_value, kernel_size=kernel_size)
                            for _ in range(depths[i])]) for i in range(len(depths)))
        self.norm = LayerNorm(dims[-1], eps=1e-6, data_format="channels_first")
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, (nn.Conv1d, nn.Linear)):
            nn.init.trunc_normal_(m.weight, std=0.02)
            nn.init.constant_(m.bias, 0)


def get_padding(kernel_size, dilation=1):
    return (kernel_size * dilation - dilation) // 2


class ResBlock1(_ParamsOnly):
    """head.py:25-99: one conv pair per dilation (the reference has three)."""
    def __init__(self, channels, kernel_size=3, dilation=(1, 3, 5)):
        super().__init__()
        self.convs1 = nn.ModuleList(weight_norm(nn.Conv1d(channels, channels, kernel_size, 1, dilation=d,
                                                          padding=get_padding(kernel_size, d))) for d in dilation)
        self.convs2 = nn.ModuleList(weight_norm(nn.Conv1d(channels, channels, kernel_size, 1, dilation=1,
                                                          padding=get_padding(kernel_size, 1))) for _ in dilation)


class ParralelBlock(_ParamsOnly):
    """head.py:117-130."""
    def __init__(self, channels, kernel_sizes=(3, 7, 11), dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 5))):
        super().__init__()
        assert len(kernel_sizes) == len(dilation_sizes)
        self.blocks = nn.ModuleList(ResBlock1(channels, k, d) for k, d in zip(kernel_sizes, dilation_sizes))


class HiFiGANGenerator(_ParamsOnly):
    """head.py:136-224 with use_template=False (the template / noise-conv path is not built natively)."""
    def __init__(self, *, hop_length=512, upsample_rates=(8, 8, 2, 2, 2), upsample_kernel_sizes=(16, 16, 8, 2, 2),
                 resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 5)), num_mels=128,
                 upsample_initial_channel=512, use_template=True, pre_conv_kernel_size=7, post_conv_kernel_size=7):
        super().__init__()
        assert prod(upsample_rates) == hop_length, f"hop_length must be {prod(upsample_rates)}"
        if use_template:
            raise NotImplementedError("native HiFiGANGenerator is built for use_template=False (FireflyGANBase's configuration)")
        self.use_template = False
        self.num_upsamples, self.num_kernels = len(upsample_rates), len(resblock_kernel_sizes)
        self.conv_pre = weight_norm(nn.Conv1d(num_mels, upsample_initial_channel, pre_conv_kernel_size, 1,
                                              padding=get_padding(pre_conv_kernel_size)))
        self.noise_convs = nn.ModuleList()
        self.ups = nn.ModuleList(
            weight_norm(nn.ConvTranspose1d(upsample_initial_channel // (2 ** i), upsample_initial_channel // (2 ** (i + 1)), k, u,
                                           padding=(k - u) // 2)) for i, (u, k) in enumerate(zip(upsample_rates, upsample_kernel_sizes)))
        self.resblocks = nn.ModuleList(
            ParralelBlock(upsample_initial_channel // (2 ** (i + 1)), resblock_kernel_sizes, resblock_dilation_sizes)
            for i in range(len(self.ups)))
        ch = upsample_initial_channel // (2 ** len(self.ups))
        self.conv_post = weight_norm(nn.Conv1d(ch, 1, post_conv_kernel_size, 1, padding=get_padding(post_conv_kernel_size)))
        self.checkpointing = False


class FireflyGANBase(NativeModule):
    """``FireflyGANBase()`` as the reference builds it (model.py:44-50); ``config`` replaces ``config_dict`` for other
    supported shapes (include/stabletts_hip.h: st_ffgan_config names the native limits; st_create_ffgan rejects the rest).

    ``operand_dtype``: "f16" (default) or "bf16" round every MFMA operand once; "f16_split" / "bf16_split" carry each operand as a
    hi + lo pair of that format (three MFMA products, fp32 accumulation; bf16 needs four in the encoder and three parts with six
    products in the head): the waveform then sits at fp32 distance from float64 (bf16_split: 1e-5) in place of 1e-3 ... 2e-3 of
    max |audio|, at three times the MFMA work and more (README: the FireflyGAN paragraph has the timings)."""
    _what = "FireflyGAN vocoder"
    _rebind = False             # st_finalize folds the weight norm and packs the weights: every change re-loads

    def __init__(self, operand_dtype="f16", config=None):
        super().__init__()
        cfg = config or config_dict
        self.config = cfg
        self.operand_dtype = operand_dtype
        self._fields = _lib.ffgan_config_fields(cfg["backbone"], cfg["head"])
        self.input_channels = int(cfg["backbone"]["input_channels"])
        self.hop_length = prod(cfg["head"]["upsample_rates"])
        self.backbone = ConvNeXtEncoder(**cfg["backbone"])
        self.head = HiFiGANGenerator(**{"hop_length": self.hop_length, **cfg["head"]})
        # inference-only module, like Vocos: the parameters do not ask for gradients; asking for them raises in forward
        self.requires_grad_(False)

    def _create_engine(self, dev):
        return _lib.Engine(0, 0, 0, 0, 0, 0, 0, self.operand_dtype, dev, ffgan=self._fields)

    def forward(self, x):
        """mel (B, input_channels, T) -> audio (B, T * hop_length)  (model.py:52-57)."""
        return self._vocode(x, None)

    def forward_ragged(self, x, lengths):
        """``forward`` for a padded batch whose utterance b has ``lengths[b]`` frames (e.g. ``synthesise``'s mel with its
        ``y_lengths``): mel (B, input_channels, T), lengths B ints in [1, T] (a sequence, or an integer tensor: a device tensor
        costs one ``.tolist()`` sync) -> audio (B, T * hop_length).  Each utterance's audio is what ``forward`` gives for it alone;
        ``audio[b, lengths[b] * hop_length:]`` is 0.  ``forward`` has no mask (like the reference), so there the padding reaches
        back through the encoder's and the head's convolutions into the end of every shorter utterance."""
        return self._vocode(x, host_lengths(lengths, x))

    def _vocode(self, x, lengths):
        if x.device.type != "cuda":
            raise ValueError(f"mel is on {x.device}: the native FireflyGAN vocoder runs only on a HIP device (there is no CPU fallback)")
        if x.dim() != 3 or x.shape[1] != self.input_channels:
            raise ValueError("mel must be (B, input_channels, T)")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("the native FireflyGAN vocoder is inference-only: it has no backward, so a mel or parameters "
                                      "that require grad would silently train nothing; run it under torch.no_grad()")
        dev = next(self.parameters()).device
        if x.device != dev:
            raise ValueError(f"mel is on {x.device}, the vocoder's parameters are on {dev}")
        with torch.no_grad():
            eng = self.engine()
            mel = x.detach().to(torch.float32).contiguous()
            B, _, T = mel.shape
            audio = torch.empty(B, T * self.hop_length, device=dev, dtype=torch.float32)
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                if lengths is None:
                    eng.ffgan_forward(mel, audio, stream)
                else:
                    eng.ffgan_forward_ragged(mel, lengths, audio, stream)
            return audio


class FireflyGANBaseWrapper(nn.Module):
    """model.py:32-42: loads the generator checkpoint (the fishaudio ``firefly-gan-base-generator.ckpt`` layout) strictly."""
    def __init__(self, model_path, operand_dtype="f16"):
        super().__init__()
        self.model = FireflyGANBase(operand_dtype=operand_dtype)
        self.model.load_state_dict(torch.load(model_path, weights_only=True, map_location="cpu"))
        self.model.eval()

    @torch.inference_mode()
    def forward(self, x):
        return self.model(x)

    @torch.inference_mode()
    def forward_ragged(self, x, lengths):
        return self.model.forward_ragged(x, lengths)
