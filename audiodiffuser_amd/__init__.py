"""MI355X-native EDM sampling hot path of AudioDiffuser.

Plugin surface (hydra ``_target_`` s): ``audiodiffuser_amd.UNet1dBase`` / ``audiodiffuser_amd.WaveNetNoise`` / ``audiodiffuser_amd.UNetModel`` /
``audiodiffuser_amd.UNet2dBase`` / ``audiodiffuser_amd.DiT`` (the adaLN-Zero transformer, exact fp32) (model.net),
``audiodiffuser_amd.EluDiffusion`` / ``VEDiffusion`` / ``VPDiffusion`` / ``VDiffusion`` / ``ReFlow`` (model.diffusion), ``audiodiffuser_amd.EDMSampler`` /
``EDMAlphaSampler`` / ``DPMSampler`` / ``DPM2Sampler`` / ``DPM2MSampler`` / ``ADPM2Sampler`` / ``ADPMPP2SSampler`` / ``LMSSampler`` / ``UniPCSampler`` /
``ReflowEulerSampler`` / ``VESampler`` / ``VPSampler`` / ``VSampler`` / ``VEulerSampler`` / ``VDPMSampler`` / ``VUniPCSampler`` (model.sampler), ``audiodiffuser_amd.KarrasSchedule`` / ``VESchedule`` / ``VPSchedule`` / ``VSchedule`` / ``LinearSchedule`` /
``GeometricSchedule`` / ``RFEDMSchedule`` (model.noise_scheduler), ``audiodiffuser_amd.LogNormalDistribution`` / ``UniformDistribution`` /
``LogUniformDistribution`` / ``LogitDistribution`` (model.noise_distribution), ``audiodiffuser_amd.SpecToWave`` (the sampled complex spectrogram to audio: spec_back + inverse STFT),
``audiodiffuser_amd.WaveToSpec`` (a waveform to that spectrogram: STFT + spec_fwd), ``audiodiffuser_amd.DACDecoder`` / ``FineTuneAutoencoder`` (a sampled
latent to audio: the autoencoder's decode stack and the DAC decoder, exact fp32), ``audiodiffuser_amd.DACEncoder`` (audio to the DAC embedding; with
``FineTuneAutoencoder.encode(x, is_train=False)`` the latent and its KL term).
"""
from .config import UNet1dConfig, config_c1, config_c2, config_c3, config_tiny, config_tiny_cc, PRESETS  # noqa: F401
from .config import WaveNetConfig, config_c5, config_c5_small  # noqa: F401
from .scheduler import KarrasSchedule, LinearSchedule, GeometricSchedule, VPSchedule, VESchedule, VSchedule, RFEDMSchedule  # noqa: F401
from .distribution import LogNormalDistribution, UniformDistribution, LogUniformDistribution, LogitDistribution  # noqa: F401
from .net import UNet1dBase  # noqa: F401
from .wavenet import WaveNetNoise  # noqa: F401
from .adm import UNetModel  # noqa: F401
from .adm_config import ADMConfig, config_c4, config_c4_small  # noqa: F401
from .unet2d import UNet2dBase  # noqa: F401
from .unet2d_config import UNet2dConfig  # noqa: F401
from .dit import DiT, DiTConfig  # noqa: F401
from .dac import DACDecoder, DACEncoder, FineTuneAutoencoder, DACConfig  # noqa: F401
from .diffusion import EluDiffusion, VEDiffusion, VPDiffusion, VDiffusion, ReFlow  # noqa: F401
from .samplers import EDMSampler, EDMAlphaSampler, DPMSampler, DPM2Sampler, DPM2MSampler, ADPM2Sampler, ADPMPP2SSampler, LMSSampler, UniPCSampler  # noqa: F401
from .samplers import ReflowEulerSampler, VESampler, VPSampler, VSampler, VEulerSampler, VDPMSampler, VUniPCSampler  # noqa: F401
from .spectral import SpecToWave, WaveToSpec  # noqa: F401
