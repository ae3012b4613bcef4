"""ctypes binding of libstabletts_hip.so (C ABI: include/stabletts_hip.h).

The library is built in-tree by ``python -m stabletts_amd.build`` (hipcc, gfx950).  There is
NO fallback: if the shared library is missing or fails to load, importing the native path raises.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STABLETTS_HIP_LIB") or os.path.join(HERE, "libstabletts_hip.so")   # env: developer A/B builds

ST_OK = 0
ST_ERR_INVALID, ST_ERR_HIP, ST_ERR_STATE, ST_ERR_UNSUPPORTED = -1, -2, -3, -4
ST_OPERAND_BF16, ST_OPERAND_F16, ST_OPERAND_BF16_SPLIT, ST_OPERAND_F16_SPLIT = 0, 1, 2, 3
ST_SOLVER_EULER, ST_SOLVER_MIDPOINT, ST_SOLVER_RK4, ST_SOLVER_DOPRI5 = 0, 1, 2, 3
ST_SOLVER_BOSH3, ST_SOLVER_FEHLBERG2, ST_SOLVER_ADAPTIVE_HEUN, ST_SOLVER_IMPLICIT_ADAMS = 4, 5, 6, 7
OPERAND_DTYPES = {"bf16": ST_OPERAND_BF16, "f16": ST_OPERAND_F16, "fp16": ST_OPERAND_F16,
                  "bf16_split": ST_OPERAND_BF16_SPLIT, "f16_split": ST_OPERAND_F16_SPLIT}
# hi + lo operand pairs (include/stabletts_hip.h): the FireflyGAN vocoder only
SPLIT_OPERAND_DTYPES = ("bf16_split", "f16_split")
# None is torchdiffeq's default method = dopri5 (models/flow_matching.py:54)
SOLVERS = {"euler": ST_SOLVER_EULER, "midpoint": ST_SOLVER_MIDPOINT, "rk4": ST_SOLVER_RK4,
           "dopri5": ST_SOLVER_DOPRI5, None: ST_SOLVER_DOPRI5, "bosh3": ST_SOLVER_BOSH3,
           "fehlberg2": ST_SOLVER_FEHLBERG2, "adaptive_heun": ST_SOLVER_ADAPTIVE_HEUN,
           "implicit_adams": ST_SOLVER_IMPLICIT_ADAMS}      # = every method the reference's webui.py:110 offers

ST_PAD_MODES = {"reflect": 0, "constant": 1, "replicate": 2, "circular": 3}
ST_MEL_LOG, ST_MEL_LINEAR = 0, 1
ST_LSGAN_REAL, ST_LSGAN_FAKE, ST_LSGAN_REAL_FAKE = 0, 1, 2


class StConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "noise_channels", "hidden_channels", "filter_channels", "n_heads", "n_layers",
        "kernel_size", "gin_channels", "operand_dtype")]


class StVocosConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "input_channels", "dim", "intermediate_dim", "num_layers", "n_fft", "hop_length", "operand_dtype")]


class StStyleEncoderConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "n_mel_channels", "style_hidden", "style_vector_dim", "style_kernel_size", "style_head")]


class StDurationPredictorConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("in_channels", "filter_channels", "kernel_size", "gin_channels")]


class StMelConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("n_fft", "win_length", "hop_length", "pad", "n_mels", "center", "pad_mode")]


class StPeriodDiscConfig(ctypes.Structure):
    _fields_ = [("period", ctypes.c_int32), ("lrelu_slope", ctypes.c_float)]


class StResolutionDiscConfig(ctypes.Structure):
    """st_resolution_disc_config: band_lo[5] / band_hi[5] as ten named fields (the same layout)."""
    _fields_ = ([("window_length", ctypes.c_int32)] + [(f"band_lo{c}", ctypes.c_int32) for c in range(5)]
                + [(f"band_hi{c}", ctypes.c_int32) for c in range(5)] + [("lrelu_slope", ctypes.c_float)])


class StFfganConfig(ctypes.Structure):
    """st_ffgan_config with its arrays as named fields (the same layout): depths0..7, dims0..7, upsample_rates0..7,
    upsample_kernel_sizes0..7, resblock_kernel_sizes0..3, resblock_dilation_sizes<block>_<pair>."""
    _fields_ = [(n, ctypes.c_int32) for n in (
        ["input_channels", "n_stages"] + [f"depths{i}" for i in range(8)] + [f"dims{i}" for i in range(8)] + ["kernel_size", "n_upsamples"]
        + [f"upsample_rates{i}" for i in range(8)] + [f"upsample_kernel_sizes{i}" for i in range(8)] + ["n_resblocks"]
        + [f"resblock_kernel_sizes{i}" for i in range(4)] + ["n_dilations"]
        + [f"resblock_dilation_sizes{b}_{p}" for b in range(4) for p in range(4)]
        + ["upsample_initial_channel", "pre_conv_kernel_size", "post_conv_kernel_size", "use_template", "operand_dtype"])]


def ffgan_config_fields(backbone, head):
    """The reference's ``config_dict["backbone"]`` / ``["head"]`` (vocoders/ffgan/model.py:7-29) as StFfganConfig's fields;
    ValueError where the lists do not fit the struct's arrays or each other (the native limits themselves: st_create_ffgan)."""
    depths, dims = list(backbone["depths"]), list(backbone["dims"])
    rates, kernels = list(head["upsample_rates"]), list(head["upsample_kernel_sizes"])
    rk, rd = list(head["resblock_kernel_sizes"]), [list(d) for d in head["resblock_dilation_sizes"]]
    if len(depths) != len(dims) or not 1 <= len(dims) <= 8:
        raise ValueError("backbone depths and dims must have the same length, 1..8")
    if len(rates) != len(kernels) or not 1 <= len(rates) <= 8:
        raise ValueError("head upsample_rates and upsample_kernel_sizes must have the same length, 1..8")
    if len(rk) != len(rd) or not 1 <= len(rk) <= 4:
        raise ValueError("head resblock_kernel_sizes and resblock_dilation_sizes must have the same length, 1..4")
    if len({len(d) for d in rd}) != 1 or not 1 <= len(rd[0]) <= 4:
        raise ValueError("every resblock needs the same number of dilations, 1..4")
    if int(head["num_mels"]) != dims[-1]:
        raise ValueError("the head's num_mels must be the encoder's last width")
    f = {n: 0 for n, _ in StFfganConfig._fields_}
    f.update(input_channels=backbone["input_channels"], n_stages=len(dims), kernel_size=backbone.get("kernel_size", 7),
             n_upsamples=len(rates), n_resblocks=len(rk), n_dilations=len(rd[0]),
             upsample_initial_channel=head["upsample_initial_channel"], pre_conv_kernel_size=head["pre_conv_kernel_size"],
             post_conv_kernel_size=head["post_conv_kernel_size"], use_template=int(bool(head.get("use_template", True))))
    for i, (a, b) in enumerate(zip(depths, dims)):
        f[f"depths{i}"], f[f"dims{i}"] = a, b
    for i, (a, b) in enumerate(zip(rates, kernels)):
        f[f"upsample_rates{i}"], f[f"upsample_kernel_sizes{i}"] = a, b
    for b, (k, ds) in enumerate(zip(rk, rd)):
        f[f"resblock_kernel_sizes{b}"] = k
        for p, d in enumerate(ds):
            f[f"resblock_dilation_sizes{b}_{p}"] = d
    return f


# Engine(...) keyword whose value is a configuration dict -> (its struct, the creator it goes to); in the order Engine looks
CREATORS = {"mel": (StMelConfig, "st_create_mel_extractor"), "style_encoder": (StStyleEncoderConfig, "st_create_style_encoder"),
            "duration_predictor": (StDurationPredictorConfig, "st_create_duration_predictor"),
            "vocoder": (StVocosConfig, "st_create_vocoder"),
            "period_discriminator": (StPeriodDiscConfig, "st_create_period_discriminator"),
            "resolution_discriminator": (StResolutionDiscConfig, "st_create_resolution_discriminator"),
            "ffgan": (StFfganConfig, "st_create_ffgan")}


class NativeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libstabletts_hip error {code}: {msg}")
        self.code = code


vp, i32, i64, u64, f32, f64, c_char_p, P = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float,
                                              ctypes.c_double, ctypes.c_char_p, ctypes.POINTER)
# Every symbol include/stabletts_hip.h declares: name -> (restype, argtypes).  load() sets the prototypes from it, so a symbol
# cannot be exported without one.
PROTOTYPES = {
    "st_abi_version": (i32, []),
    "st_create": (i32, [P(StConfig), i32, P(vp)]),
    "st_destroy": (None, [vp]),
    "st_last_error": (c_char_p, [vp]),
    "st_load_param": (i32, [vp, c_char_p, vp, P(i64), i32]),
    "st_num_params": (i32, [vp]),
    "st_finalize": (i32, [vp]),
    "st_bind_param": (i32, [vp, c_char_p, vp, P(i64), i32]),
    "st_repack": (i32, [vp, vp]),
    "st_train_serial": (i64, [vp]),
    "st_estimator_forward": (i32, [vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, vp]),
    "st_cfm_solve": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, i32, i32, vp]),
    "st_output_status": (i32, [vp, vp, P(i32)]),
    "st_last_solve_stats": (i32, [vp] + [P(i64)] * 3),
    "st_debug_capture": (i32, [vp, i32]),
    "st_debug_fetch": (i64, [vp, c_char_p, vp, i64]),
    "st_profile_enable": (i32, [vp, i32]),
    "st_profile_select": (i32, [vp, u64]),
    "st_param_info": (i32, [vp, i32, P(c_char_p), P(i64)]),
    "st_create_text_encoder": (i32, [P(StConfig), i32, i32, P(vp)]),
    "st_text_encoder_forward": (i32, [vp] + [vp] * 6 + [i32, i32, vp]),
    "st_profile_stride": (i32, [vp, i32]),
    "st_profile_num_classes": (i32, []),
    "st_profile_class_name": (c_char_p, [i32]),
    "st_profile_read": (i32, [vp, i32, P(i64), P(f64), P(f64)]),
    "st_device_bytes": (i64, [vp]),
    "st_train_forward": (i32, [vp] + [vp] * 6 + [i32, i32, f32, u64, vp]),
    "st_train_backward": (i32, [vp, i64, i32, i32] + [vp] * 4 + [vp]),
    "st_train_backward_part": (i32, [vp, i64, i32, i32, i32, vp, vp, i64] + [vp] * 3 + [vp]),
    "st_text_encoder_train_forward": (i32, [vp] + [vp] * 6 + [i32, i32, f32, u64, vp]),
    "st_text_encoder_train_backward": (i32, [vp, i64, i32, i32] + [vp] * 4 + [vp]),
    "st_train_param_part": (i32, [vp, c_char_p]),
    "st_train_grad_offset": (i64, [vp, c_char_p]),
    "st_train_grad_numel": (i64, [vp]),
    "st_param_grad": (i32, [vp, c_char_p, vp, i64, vp]),
    "st_param_grads_flat": (i32, [vp, vp, i64, vp]),
    "st_durations": (i32, [vp, vp, f32, i32, i32, vp, vp, vp, vp]),
    "st_generate_path": (i32, [vp, vp, i32, i32, i32, vp, vp, vp]),
    "st_align": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "st_cfm_loss_prep": (i32, [vp, vp, vp, f32, i32, i32, i32, vp, vp, vp, vp]),
    "st_cfm_loss": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "st_cfm_loss_backward": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp]),
    "st_cfm_loss_scratch_floats": (i32, []),
    "st_create_vocoder": (i32, [P(StVocosConfig), i32, P(vp)]),
    "st_vocos_forward": (i32, [vp, vp, vp, i32, i32, vp]),
    "st_vocos_forward_ragged": (i32, [vp, vp, P(i64), vp, i32, i32, vp]),
    "st_vocos_train_forward": (i32, [vp, vp, vp, i32, i32, vp]),
    "st_vocos_train_backward": (i32, [vp, vp, vp, vp, i32, i32, vp]),
    "st_create_ffgan": (i32, [P(StFfganConfig), i32, P(vp)]),
    "st_ffgan_forward": (i32, [vp, vp, vp, i32, i32, vp]),
    "st_ffgan_forward_ragged": (i32, [vp, vp, P(i64), vp, i32, i32, vp]),
    "st_create_period_discriminator": (i32, [P(StPeriodDiscConfig), i32, P(vp)]),
    "st_period_disc_fmap_shape": (i32, [vp, i32, i32, P(i64), P(i64)]),
    "st_period_disc_forward": (i32, [vp, vp, P(vp), i32, i32, vp]),
    "st_period_disc_train_forward": (i32, [vp, vp, P(vp), i32, i32, vp]),
    "st_period_disc_train_backward": (i32, [vp, P(vp), vp, vp, i32, i32, vp]),
    "st_create_resolution_discriminator": (i32, [P(StResolutionDiscConfig), i32, P(vp)]),
    "st_resolution_disc_fmap_shape": (i32, [vp, i32, i32, P(i64), P(i64), P(i64)]),
    "st_resolution_disc_wgrad_planes": (i32, [vp, i32, i32, i32, i32]),
    "st_resolution_disc_forward": (i32, [vp, vp, P(vp), i32, i32, vp]),
    "st_resolution_disc_train_forward": (i32, [vp, vp, P(vp), i32, i32, vp]),
    "st_resolution_disc_train_backward": (i32, [vp, P(vp), vp, vp, i32, i32, vp]),
    "st_set_option": (i32, [vp, c_char_p, i32]),
    "st_get_option": (i32, [vp, c_char_p, P(i32)]),
    "st_attention_stats": (i32, [vp, vp, P(f32)]),
    "st_create_style_encoder": (i32, [P(StStyleEncoderConfig), i32, P(vp)]),
    "st_style_encoder_forward": (i32, [vp, vp, vp, vp, i32, i32, vp]),
    "st_create_duration_predictor": (i32, [P(StDurationPredictorConfig), i32, P(vp)]),
    "st_duration_predictor_forward": (i32, [vp, vp, vp, vp, vp, i32, i32, vp]),
    "st_style_encoder_train_forward": (i32, [vp, vp, vp, vp, i32, i32, f32, u64, vp]),
    "st_style_encoder_train_backward": (i32, [vp, i64, i32, i32, vp, vp, vp]),
    "st_duration_predictor_train_forward": (i32, [vp] + [vp] * 4 + [i32, i32, f32, u64, vp]),
    "st_duration_predictor_train_backward": (i32, [vp, i64, i32, i32, vp, vp, vp]),
    "st_maximum_path": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "st_maximum_path_workspace_bytes": (i64, [i32, i32, i32]),
    "st_mas_neg_cent": (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
    "st_align_train_scratch_floats": (i32, [i32, i32, i32]),
    "st_align_train_forward": (i32, [vp] * 7 + [i32] * 4 + [vp] * 5 + [vp]),
    "st_align_train_backward": (i32, [vp] * 10 + [i32] * 4 + [vp] * 2 + [vp]),
    "st_duration_loss": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    "st_duration_loss_backward": (i32, [vp, vp, vp, vp, vp, i32, i32, vp, vp]),
    "st_duration_loss_scratch_floats": (i32, []),
    "st_gan_loss_chunk": (i32, []),
    "st_gan_loss_max_pairs": (i32, []),
    "st_gan_loss_scratch_bytes": (i64, [P(i64), i32]),
    "st_feature_loss_forward": (i32, [P(vp), P(vp), P(i64), i32, vp, vp, i64, vp]),
    "st_feature_loss_backward": (i32, [P(vp), P(vp), P(i64), i32, vp, P(vp), P(vp), vp]),
    "st_lsgan_loss_forward": (i32, [P(vp), P(i64), i32, i32, vp, vp, i64, vp]),
    "st_lsgan_loss_backward": (i32, [P(vp), P(i64), i32, i32, vp, P(vp), vp]),
    "st_optim_chunk": (i32, []),
    "st_optim_max_tensors": (i32, []),
    "st_grad_norm_scratch_bytes": (i64, [P(i64), i32]),
    "st_grad_norm": (i32, [P(vp), P(i64), i32, vp, vp, i64, vp]),
    "st_grad_clip": (i32, [P(vp), P(i64), i32, vp, f32, vp]),
    "st_adamw_step": (i32, [P(vp), P(vp), P(vp), P(vp), P(i64), P(i64), i32, f64, f64, f64, f64, f64, vp]),
    "st_resample_chunk": (i32, []),
    "st_resample_max_tensors": (i32, []),
    "st_resample": (i32, [P(vp), P(vp), P(i64), P(i64), i32, i32, i32, vp, vp, i32, vp]),
    "st_create_mel_extractor": (i32, [P(StMelConfig), i32, P(vp)]),
    "st_mel_frames": (i64, [vp, i64]),
    "st_mel_forward": (i32, [vp, vp, i32, i64, vp, vp]),
    "st_mel_forward_ragged": (i32, [vp, vp, P(i64), P(i64), i32, i32, vp, vp]),
    "st_mel_backward_workspace_bytes": (i64, [vp, i32, i64]),
    "st_mel_backward": (i32, [vp, vp, vp, i32, i64, i32, vp, vp, vp]),
}
EXPORTS = list(PROTOTYPES)


_lib = None


def load():
    """Loads the shared library (once).  torch is imported first so that the HIP runtime the
    library binds to (SONAME libamdhip64.so.7) is the one torch already loaded: a process must
    not hold two HIP runtimes, streams and device pointers are shared across the boundary."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401  (loads torch/lib/libamdhip64.so when the wheel bundles it)
        tl = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(tl):
            ctypes.CDLL(tl, mode=ctypes.RTLD_GLOBAL)
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build it with `python -m stabletts_amd.build` "
                          "(the native HIP path has no fallback)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.st_abi_version() != 4:
        raise ImportError("libstabletts_hip.so ABI version mismatch; rebuild it")
    _lib = lib
    return lib


class Engine:
    """Thin owner of one ``st_engine`` handle."""

    def __init__(self, noise_channels, hidden_channels, filter_channels, n_heads, n_layers, kernel_size,
                 gin_channels, operand_dtype="f16", device=0, text_encoder_vocab=None, vocoder=None,
                 style_encoder=None, duration_predictor=None, mel=None, period_discriminator=None, resolution_discriminator=None,
                 ffgan=None):
        """text_encoder_vocab: None -> CFM decoder estimator (st_create); n_vocab -> TextEncoder handle
        (st_create_text_encoder; noise_channels is then the encoder's out_channels).
        vocoder: dict(input_channels, dim, intermediate_dim, num_layers, n_fft, hop_length) -> Vocos handle
        (st_create_vocoder; the decoder arguments are ignored).
        style_encoder: dict(n_mel_channels, style_hidden, style_vector_dim, style_kernel_size, style_head) -> MelStyleEncoder
        handle (st_create_style_encoder); duration_predictor: dict(in_channels, filter_channels, kernel_size, gin_channels)
        -> DurationPredictor handle (st_create_duration_predictor).  Both fp32: the decoder arguments are ignored.
        mel: dict(n_fft, win_length, hop_length, pad, n_mels, center, pad_mode) -> mel-extractor handle (st_create_mel_extractor;
        pad_mode an ST_PAD_* value, n_mels 0 for a linear spectrogram).
        period_discriminator: dict(period, lrelu_slope) -> DiscriminatorP handle (st_create_period_discriminator), fp32.
        resolution_discriminator: dict(window_length, band_lo0..4, band_hi0..4, lrelu_slope) -> DiscriminatorR handle
        (st_create_resolution_discriminator), fp32.
        ffgan: the fields of StFfganConfig (ffgan_config_fields) -> FireflyGAN vocoder handle (st_create_ffgan)."""
        self.lib = load()
        if operand_dtype not in OPERAND_DTYPES:
            raise ValueError(f"operand_dtype must be one of {sorted(OPERAND_DTYPES)}")
        self.operand_dtype = operand_dtype
        h = ctypes.c_void_p()
        dicts = dict(mel=mel, style_encoder=style_encoder, duration_predictor=duration_predictor, vocoder=vocoder,
                     period_discriminator=period_discriminator, resolution_discriminator=resolution_discriminator, ffgan=ffgan)
        kw = next((k for k in CREATORS if dicts[k] is not None), None)
        if operand_dtype in SPLIT_OPERAND_DTYPES and kw != "ffgan":      # no st_create_* but st_create_ffgan knows the value
            raise ValueError(f"operand_dtype {operand_dtype!r} (hi + lo operand pairs) exists for the FireflyGAN vocoder only")
        if kw:          # a configuration dict: its struct's fields by name (operand_dtype, where the struct has one, from the argument)
            (struct, creator), d = CREATORS[kw], dicts[kw]
            cfg = struct(*(OPERAND_DTYPES[operand_dtype] if n == "operand_dtype" else (float if t is ctypes.c_float else int)(d[n])
                           for n, t in struct._fields_))
            rc = getattr(self.lib, creator)(ctypes.byref(cfg), int(device), ctypes.byref(h))
        else:
            cfg = StConfig(noise_channels, hidden_channels, filter_channels, n_heads, n_layers, kernel_size,
                           gin_channels, OPERAND_DTYPES[operand_dtype])
            if text_encoder_vocab is None:
                rc = self.lib.st_create(ctypes.byref(cfg), int(device), ctypes.byref(h))
            else:
                rc = self.lib.st_create_text_encoder(ctypes.byref(cfg), int(text_encoder_vocab), int(device), ctypes.byref(h))
        if rc != ST_OK:
            raise NativeError(rc, self.lib.st_last_error(None).decode())
        self.handle = h
        self.device = int(device)

    def _check(self, rc):
        if rc != ST_OK:
            raise NativeError(rc, self.lib.st_last_error(self.handle).decode())

    def close(self):
        if getattr(self, "handle", None):
            self.lib.st_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def num_params(self):
        return self.lib.st_num_params(self.handle)

    def param_info(self):
        """[(reference state_dict name, shape)] the handle expects, in the engine's (name) order."""
        out = []
        for i in range(self.num_params()):
            name = ctypes.c_char_p()
            shape = (ctypes.c_int64 * 4)()
            nd = self.lib.st_param_info(self.handle, i, ctypes.byref(name), shape)
            if nd < 0:
                raise NativeError(nd, "st_param_info")
            out.append((name.value.decode(), tuple(shape[:nd])))
        return out

    def load_state_dict(self, sd):
        """sd: name -> torch.Tensor (fp32, any device), reference ``decoder.estimator.*`` names."""
        for name, t in sd.items():
            t = t.detach().float().contiguous()
            shape = (ctypes.c_int64 * t.dim())(*t.shape)
            self._check(self.lib.st_load_param(self.handle, name.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim()))
        self._check(self.lib.st_finalize(self.handle))

    def bind_parameters(self, named_params):
        """named_params: iterable of (reference name, fp32 contiguous tensor ON THE ENGINE'S DEVICE).  The engine reads
        the tensors in place from now on (st_bind_param: no copy; the caller keeps them alive) and packs its 16-bit
        operand copies (st_finalize)."""
        for name, t in named_params:
            shape = (ctypes.c_int64 * t.dim())(*t.shape)
            self._check(self.lib.st_bind_param(self.handle, name.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim()))
        self._check(self.lib.st_finalize(self.handle))

    def repack(self, stream):
        """After an in-place update of the bound tensors: re-pack the 16-bit copies as kernels on ``stream`` (no sync)."""
        self._check(self.lib.st_repack(self.handle, ctypes.c_void_p(stream)))

    def estimator_forward(self, t, x, mu, mask, c, out, stream):
        B, _, T = x.shape
        self._check(self.lib.st_estimator_forward(self.handle, t.data_ptr(), int(t.numel()), x.data_ptr(), mu.data_ptr(),
                                                  mask.data_ptr(), c.data_ptr(), out.data_ptr(), B, T,
                                                  ctypes.c_void_p(stream)))

    def cfm_solve(self, mu, mask, z, c, n_steps, solver, use_cfg, cfg_strength, fake_speaker, fake_content, out, stream):
        B, _, T = mu.shape
        self._check(self.lib.st_cfm_solve(self.handle, mu.data_ptr(), mask.data_ptr(), z.data_ptr(), c.data_ptr(),
                                          int(n_steps), int(solver), int(bool(use_cfg)), float(cfg_strength),
                                          fake_speaker.data_ptr() if fake_speaker is not None else None,
                                          fake_content.data_ptr() if fake_content is not None else None,
                                          out.data_ptr(), B, T, ctypes.c_void_p(stream)))

    def text_encoder_forward(self, tokens, lengths, c, x_out, mu_out, mask_out, stream):
        B, T = tokens.shape
        self._check(self.lib.st_text_encoder_forward(self.handle, tokens.data_ptr(), lengths.data_ptr(), c.data_ptr(),
                                                     x_out.data_ptr(), mu_out.data_ptr(), mask_out.data_ptr(), B, T,
                                                     ctypes.c_void_p(stream)))

    def _vocoder_forward(self, fn, mel, lengths, audio, stream):
        """mel (B, input_channels, T) -> audio (B, T * hop); lengths (a sequence of B ints, host side): the ragged entry point `fn`."""
        B, _, T = mel.shape
        if lengths is None:
            return self._check(fn(self.handle, mel.data_ptr(), audio.data_ptr(), B, T, ctypes.c_void_p(stream)))
        if len(lengths) != B:
            raise NativeError(ST_ERR_INVALID, f"lengths has {len(lengths)} entries, the batch has B = {B} utterances")
        arr = (ctypes.c_int64 * B)(*lengths)
        self._check(fn(self.handle, mel.data_ptr(), arr, audio.data_ptr(), B, T, ctypes.c_void_p(stream)))

    def vocos_forward(self, mel, audio, stream):
        self._vocoder_forward(self.lib.st_vocos_forward, mel, None, audio, stream)

    def ffgan_forward(self, mel, audio, stream):
        """mel (B, input_channels, T) -> audio (B, T * hop) (FireflyGAN vocoder handles)."""
        self._vocoder_forward(self.lib.st_ffgan_forward, mel, None, audio, stream)

    def ffgan_forward_ragged(self, mel, lengths, audio, stream):
        """st_ffgan_forward with utterance b at its own length lengths[b] (a sequence of B ints, host side)."""
        self._vocoder_forward(self.lib.st_ffgan_forward_ragged, mel, lengths, audio, stream)

    def vocos_forward_ragged(self, mel, lengths, audio, stream):
        """st_vocos_forward with utterance b at its own length lengths[b] (a sequence of B ints, host side)."""
        self._vocoder_forward(self.lib.st_vocos_forward_ragged, mel, lengths, audio, stream)

    def vocos_train_forward(self, mel, audio, stream):
        """st_vocos_forward in fp32 that keeps the activations for vocos_train_backward (vocoder handles)."""
        B, _, T = mel.shape
        self._check(self.lib.st_vocos_train_forward(self.handle, mel.data_ptr(), audio.data_ptr(), B, T, ctypes.c_void_p(stream)))

    def vocos_train_backward(self, B, T, d_audio, d_mel, grad_flat, stream):
        """Every parameter gradient into grad_flat (grad_layout()[None] floats) and d mel (None: not wanted) from d loss / d audio."""
        if grad_flat.numel() != self.grad_layout()[None]:
            raise ValueError("grad_flat must hold grad_layout()[None] floats")
        self._check(self.lib.st_vocos_train_backward(self.handle, d_audio.data_ptr(), d_mel.data_ptr() if d_mel is not None else None,
                                                     grad_flat.data_ptr(), B, T, ctypes.c_void_p(stream)))

    def _disc_fmap_shapes(self, fn, n, B, T, n_dims, too_short):
        """(B, *dims) of each of the n feature maps; `too_short`: the message when T is below the kind's minimum."""
        out = []
        for i in range(n):
            dims = [ctypes.c_int64() for _ in range(n_dims)]
            if fn(self.handle, int(T), i, *[ctypes.byref(d) for d in dims]) != ST_OK:
                raise NativeError(ST_ERR_INVALID, too_short)
            out.append((B, *[d.value for d in dims]))
        return out

    def _disc_forward(self, kind, n, x, fmaps, train, stream):
        B, _, T = x.shape
        ptrs = (ctypes.c_void_p * n)(*[f.data_ptr() for f in fmaps])
        fn = getattr(self.lib, f"st_{kind}_train_forward" if train else f"st_{kind}_forward")
        self._check(fn(self.handle, x.data_ptr(), ptrs, B, T, ctypes.c_void_p(stream)))

    def _disc_train_backward(self, kind, n, B, T, d_fmaps, d_x, grad_flat, stream):
        if grad_flat is not None and grad_flat.numel() != self.grad_layout()[None]:
            raise ValueError("grad_flat must hold grad_layout()[None] floats")
        ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        ptrs = (ctypes.c_void_p * n)(*[ptr(f) for f in d_fmaps])
        self._check(getattr(self.lib, f"st_{kind}_train_backward")(self.handle, ptrs, ptr(d_x), ptr(grad_flat), B, T, ctypes.c_void_p(stream)))

    def period_disc_fmap_shapes(self, B, T, period):
        """The five feature-map shapes (B, C, H, period) of a (B, 1, T) input (period-discriminator handles)."""
        n_pad = (period - T % period) % period
        shapes = self._disc_fmap_shapes(self.lib.st_period_disc_fmap_shape, 5, B, T, 2,
                                        f"T = {T} is too short for period {period}: the reflect padding of {n_pad} samples needs T > {n_pad}")
        return [s + (period,) for s in shapes]

    def period_disc_forward(self, x, fmaps, train, stream):
        """x (B, 1, T) -> the five feature maps; train: keep the activations for period_disc_train_backward."""
        self._disc_forward("period_disc", 5, x, fmaps, train, stream)

    def period_disc_train_backward(self, B, T, d_fmaps, d_x, grad_flat, stream):
        """d_fmaps: five tensors or None each; d x (None: not wanted) and every parameter gradient into grad_flat (None: none wanted)."""
        self._disc_train_backward("period_disc", 5, B, T, d_fmaps, d_x, grad_flat, stream)

    def resolution_disc_fmap_shapes(self, B, T):
        """The 21 feature-map shapes (B, C, frames, width) of a (B, 1, T) input (resolution-discriminator handles)."""
        return self._disc_fmap_shapes(self.lib.st_resolution_disc_fmap_shape, 21, B, T, 3,
                                      f"T = {T} is too short for this window length: the reflect padding needs T > window_length / 2")

    def resolution_disc_wgrad_planes(self, B, T, band, layer):
        """Split-K planes of the weight-gradient launch of band_convs.{band}.{layer} at (B, T) (tests / tools)."""
        n = int(self.lib.st_resolution_disc_wgrad_planes(self.handle, int(B), int(T), int(band), int(layer)))
        if n < 1:
            raise NativeError(n, f"st_resolution_disc_wgrad_planes(B={B}, T={T}, band={band}, layer={layer})")
        return n

    def resolution_disc_forward(self, x, fmaps, train, stream):
        """x (B, 1, T) -> the 21 feature maps; train: keep the activations for resolution_disc_train_backward."""
        self._disc_forward("resolution_disc", 21, x, fmaps, train, stream)

    def resolution_disc_train_backward(self, B, T, d_fmaps, d_x, grad_flat, stream):
        """d_fmaps: 21 tensors or None each; d x (None: not wanted) and every parameter gradient into grad_flat (None: none wanted)."""
        self._disc_train_backward("resolution_disc", 21, B, T, d_fmaps, d_x, grad_flat, stream)

    def finalize(self):
        """st_finalize on the parameters already loaded / bound: a vocoder handle packs its 16-bit inference copies again."""
        self._check(self.lib.st_finalize(self.handle))

    def mel_frames(self, L):
        """Frames of an utterance of L samples (mel-extractor handles); raises NativeError where the reference raises."""
        n = int(self.lib.st_mel_frames(self.handle, int(L)))
        if n < 0:
            raise NativeError(n, f"no frames for an utterance of {L} samples (needs L > pad and L + 2 pad >= n_fft)")
        return n

    def mel_forward(self, wave, out, stream):
        """wave (B, L) -> out (B, n_mels, frames), log-mel."""
        B, L = wave.shape
        self._check(self.lib.st_mel_forward(self.handle, wave.data_ptr(), B, L, out.data_ptr(), ctypes.c_void_p(stream)))

    def mel_forward_ragged(self, wave, sample_offsets, frame_offsets, output, out, stream):
        """Concatenated waveforms and host offsets (B + 1 each) -> concatenated (rows, frames_b) blocks in out."""
        B = len(sample_offsets) - 1
        so = (ctypes.c_int64 * (B + 1))(*sample_offsets)
        fo = (ctypes.c_int64 * (B + 1))(*frame_offsets)
        self._check(self.lib.st_mel_forward_ragged(self.handle, wave.data_ptr(), so, fo, B, int(output), out.data_ptr(),
                                                   ctypes.c_void_p(stream)))

    def mel_backward_workspace_bytes(self, B, L):
        """Bytes of the caller-owned workspace st_mel_backward needs for a (B, L) batch."""
        n = int(self.lib.st_mel_backward_workspace_bytes(self.handle, int(B), int(L)))
        if n < 0:
            raise NativeError(n, f"no mel backward for B = {B} x L = {L}")
        return n

    def mel_backward(self, wave, grad_out, output, grad_wave, workspace, stream):
        """wave (B, L) and the gradient of the (log-mel or linear) output -> grad_wave (B, L), overwritten."""
        B, L = wave.shape
        self._check(self.lib.st_mel_backward(self.handle, wave.data_ptr(), grad_out.data_ptr(), B, L, int(output),
                                             grad_wave.data_ptr(), workspace.data_ptr(), ctypes.c_void_p(stream)))

    def style_encoder_forward(self, mel, mask, c_out, stream):
        B, _, T = mel.shape
        self._check(self.lib.st_style_encoder_forward(self.handle, mel.data_ptr(), mask.data_ptr() if mask is not None else None,
                                                      c_out.data_ptr(), B, T, ctypes.c_void_p(stream)))

    def duration_predictor_forward(self, x, x_mask, g, logw_out, stream):
        B, _, T = x.shape
        self._check(self.lib.st_duration_predictor_forward(self.handle, x.data_ptr(), x_mask.data_ptr(), g.data_ptr(),
                                                           logw_out.data_ptr(), B, T, ctypes.c_void_p(stream)))

    def style_encoder_train_forward(self, mel, mask, c_out, p_dropout, seed, stream):
        """st_style_encoder_forward that keeps the activations for style_encoder_train_backward (style-encoder handles)."""
        B, _, T = mel.shape
        self._check(self.lib.st_style_encoder_train_forward(self.handle, mel.data_ptr(), mask.data_ptr() if mask is not None else None,
                                                            c_out.data_ptr(), B, T, float(p_dropout), int(seed), ctypes.c_void_p(stream)))

    def style_encoder_train_backward(self, serial, B, T, grad_c, grad_flat, stream):
        """Every parameter gradient into grad_flat (grad_layout()[None] floats) from d loss / d c."""
        if grad_flat.numel() != self.grad_layout()[None]:
            raise ValueError("grad_flat must hold grad_layout()[None] floats")
        self._check(self.lib.st_style_encoder_train_backward(self.handle, int(serial), B, T, grad_c.data_ptr(), grad_flat.data_ptr(),
                                                             ctypes.c_void_p(stream)))

    def duration_predictor_train_forward(self, x, x_mask, g, logw_out, p_dropout, seed, stream):
        """st_duration_predictor_forward that keeps the activations for duration_predictor_train_backward."""
        B, _, T = x.shape
        self._check(self.lib.st_duration_predictor_train_forward(self.handle, x.data_ptr(), x_mask.data_ptr(), g.data_ptr(),
                                                                 logw_out.data_ptr(), B, T, float(p_dropout), int(seed),
                                                                 ctypes.c_void_p(stream)))

    def duration_predictor_train_backward(self, serial, B, T, grad_logw, grad_flat, stream):
        """Every parameter gradient into grad_flat (grad_layout()[None] floats) from d loss / d logw."""
        if grad_flat.numel() != self.grad_layout()[None]:
            raise ValueError("grad_flat must hold grad_layout()[None] floats")
        self._check(self.lib.st_duration_predictor_train_backward(self.handle, int(serial), B, T, grad_logw.data_ptr(),
                                                                  grad_flat.data_ptr(), ctypes.c_void_p(stream)))

    # ---- training: forward that keeps activations + backward (include/stabletts_hip.h, "training")
    def train_forward(self, t, x, mu, mask, c, out, p_dropout, seed, stream):
        B, _, T = x.shape
        self._check(self.lib.st_train_forward(self.handle, t.data_ptr(), x.data_ptr(), mu.data_ptr(), mask.data_ptr(),
                                              c.data_ptr(), out.data_ptr(), B, T, float(p_dropout), int(seed),
                                              ctypes.c_void_p(stream)))

    def text_encoder_train_forward(self, tokens, lengths, c, x_out, mu_out, mask_out, p_dropout, seed, stream):
        """st_text_encoder_forward that keeps the activations for text_encoder_train_backward (text-encoder handles)."""
        B, T = tokens.shape
        self._check(self.lib.st_text_encoder_train_forward(self.handle, tokens.data_ptr(), lengths.data_ptr(), c.data_ptr(),
                                                           x_out.data_ptr(), mu_out.data_ptr(), mask_out.data_ptr(), B, T,
                                                           float(p_dropout), int(seed), ctypes.c_void_p(stream)))

    def text_encoder_train_backward(self, serial, B, T, grad_x, grad_mu, grad_flat, grad_c, stream):
        """Every parameter gradient into grad_flat (grad_layout(); None: the engine's own buffers), d c into grad_c."""
        ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        if grad_flat is not None and grad_flat.numel() != self.grad_layout()[None]:
            raise ValueError("grad_flat must hold grad_layout()[None] floats")
        self._check(self.lib.st_text_encoder_train_backward(self.handle, int(serial), B, T, ptr(grad_x), ptr(grad_mu), ptr(grad_flat),
                                                            ptr(grad_c), ctypes.c_void_p(stream)))

    def train_serial(self):
        """Serial of the grad-enabled forward whose activations the engine holds (0: none)."""
        return int(self.lib.st_train_serial(self.handle))

    def train_backward(self, serial, grad_out, grad_x, grad_mu, grad_c, stream):
        ptr = lambda v: v.data_ptr() if v is not None else None      # noqa: E731
        B, _, T = grad_out.shape
        self._check(self.lib.st_train_backward(self.handle, int(serial), B, T, grad_out.data_ptr(), ptr(grad_x), ptr(grad_mu),
                                               ptr(grad_c), ctypes.c_void_p(stream)))

    def train_backward_part(self, serial, part, B, T, grad_out, grad_flat, grad_x, grad_mu, grad_c, stream):
        """One of the three parts of a backward (0: final_proj + upper blocks + long-skip convs, 1: lower blocks, 2: in_proj /
        prenet / time MLP + input gradients); grad_flat (part 0) receives every parameter gradient directly (grad_layout())."""
        ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        self._check(self.lib.st_train_backward_part(self.handle, int(serial), B, T, int(part), ptr(grad_out), ptr(grad_flat),
                                                    grad_flat.numel() if grad_flat is not None else 0, ptr(grad_x), ptr(grad_mu),
                                                    ptr(grad_c), ctypes.c_void_p(stream)))

    def param_part(self, name):
        """Backward part (0, 1, 2) that produces the gradient of parameter `name` (a function of the name only: cached)."""
        cache = self.__dict__.setdefault("_param_part", {})
        r = cache.get(name)
        if r is None:
            r = self.lib.st_train_param_part(self.handle, name.encode())
            if r < 0:
                raise NativeError(r, f"st_train_param_part({name})")
            cache[name] = r
        return r

    def param_grad(self, name, dst, stream):
        self._check(self.lib.st_param_grad(self.handle, name.encode(), dst.data_ptr(), dst.numel(), ctypes.c_void_p(stream)))

    def param_grads_flat(self, dst, stream):
        """Every parameter gradient in one copy: dst (fp32, grad_layout()[None] elements) in the flat layout."""
        self._check(self.lib.st_param_grads_flat(self.handle, dst.data_ptr(), dst.numel(), ctypes.c_void_p(stream)))

    def grad_layout(self):
        """{reference name: (offset, numel, shape)} of param_grads_flat's layout (cached)."""
        lay = getattr(self, "_grad_layout", None)
        if lay is None:
            lay = {}
            for name, shape in self.param_info():
                n = 1
                for d in shape:
                    n *= d
                off = self.lib.st_train_grad_offset(self.handle, name.encode())
                if off < 0:
                    raise NativeError(int(off), f"st_train_grad_offset({name})")
                lay[name] = (int(off), n, shape)       # slices start on 64-byte boundaries
            lay[None] = int(self.lib.st_train_grad_numel(self.handle))
            self._grad_layout = lay
        return lay

    def output_nonfinite(self, stream):
        """True when a call completed since the last query wrote NaN / Inf to its output (synchronises ``stream``)."""
        flag = ctypes.c_int(0)
        self._check(self.lib.st_output_status(self.handle, ctypes.c_void_p(stream), ctypes.byref(flag)))
        return bool(flag.value)

    def last_solve_stats(self):
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self.lib.st_last_solve_stats(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return dict(nfe=a.value, steps=b.value, rejects=c.value)

    # ---- test / measurement hooks
    def debug_capture(self, on):
        self._check(self.lib.st_debug_capture(self.handle, int(on)))

    def debug_fetch(self, name):
        import numpy as np
        n = self.lib.st_debug_fetch(self.handle, name.encode(), None, 0)
        if n < 0:
            raise NativeError(int(n), self.lib.st_last_error(self.handle).decode())
        buf = np.empty(int(n), dtype=np.float32)
        r = self.lib.st_debug_fetch(self.handle, name.encode(), buf.ctypes.data_as(ctypes.c_void_p), int(n))
        if r < 0:
            raise NativeError(int(r), self.lib.st_last_error(self.handle).decode())
        return buf

    def profile_enable(self, on, classes=None, stride=1):
        """classes: optional iterable of class names to restrict event recording to; stride: record every
        stride-th launch of a class only (event pairs cost ~10 us of stream time each)."""
        mask = (1 << 64) - 1
        if classes is not None:
            names = [self.lib.st_profile_class_name(i).decode() for i in range(self.lib.st_profile_num_classes())]
            mask = 0
            for c in classes:
                mask |= 1 << names.index(c)
        self._check(self.lib.st_profile_select(self.handle, mask))
        self._check(self.lib.st_profile_stride(self.handle, int(stride)))
        self._check(self.lib.st_profile_enable(self.handle, int(on)))

    def profile_read(self):
        """-> {class_name: dict(launches, total_ms, flops_per_launch)} since the last read."""
        out = {}
        for i in range(self.lib.st_profile_num_classes()):
            n, ms, fl = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
            self._check(self.lib.st_profile_read(self.handle, i, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl)))
            out[self.lib.st_profile_class_name(i).decode()] = dict(
                launches=n.value, total_ms=ms.value, flops_per_launch=fl.value)
        return out

    def device_bytes(self):
        return self.lib.st_device_bytes(self.handle)

    def set_option(self, name, value):
        """st_set_option: 'attention_precision' 0 (16-bit q / k operands) / 1 (split hi + lo operands)."""
        self._check(self.lib.st_set_option(self.handle, name.encode(), int(value)))

    def get_option(self, name):
        v = ctypes.c_int()
        self._check(self.lib.st_get_option(self.handle, name.encode(), ctypes.byref(v)))
        return v.value

    def attention_stats(self, stream):
        """Largest log-sum-exp (natural units) of any valid attention row since the last query (synchronises the stream; -inf: none)."""
        v = ctypes.c_float()
        self._check(self.lib.st_attention_stats(self.handle, ctypes.c_void_p(stream), ctypes.byref(v)))
        return float(v.value)
