"""Cases of tests/golden/vocos_rates.npz (tools/make_golden_vocos_rates.py): the Vocos generator at the ISTFT sizes and mel widths
of 16-24 kHz models -- n_fft 1024 / 512 / 256 with hop_length n_fft / 4, and mel widths 80, 96 and 16, none a multiple of 64.
Test infrastructure shared by the generator and by tests/test_vocos_rates_cpu.py.
"""

# name -> (config fields, B, T, weight seed, mel seed); the reference module is built with
# MelConfig(n_fft=N, win_length=N, hop_length=N // 4, n_mels=M)
CASES = {
    "n1024_m80": (dict(n_fft=1024, hop_length=256, input_channels=80, dim=512, intermediate_dim=256, num_layers=2), 2, 9, 151, 152),
    "n512_m96": (dict(n_fft=512, hop_length=128, input_channels=96, dim=768, intermediate_dim=256, num_layers=2), 2, 9, 161, 162),
    "n256_m16": (dict(n_fft=256, hop_length=64, input_channels=16, dim=1024, intermediate_dim=256, num_layers=1), 3, 5, 171, 172),
}

# what st_create_vocoder accepts: n_fft with hop_length == n_fft / 4, input_channels a multiple of 16 up to 192
N_FFTS = (256, 512, 1024, 2048)
MEL_WIDTHS = tuple(range(16, 193, 16))
