"""turbo-metrics_amd: MI355X-native SSIMULACRA2 / PSNR frame-pair engine (gfx950 HIP kernels behind a
C ABI) with a host-side mirror of the reference's operator interface.

  ffi     -- ctypes binding of include/turbo_metrics_hip.h (libturbometrics_hip.so, built in-tree)
  engine  -- TurboMetrics / Ssimulacra2 / FrameScores mirrors of the reference types
  synth   -- seeded synthetic frame generators used by bench.py and the tests
  xpsnr   -- ctypes binding of include/turbo_metrics_xpsnr.h (libturbometrics_xpsnr.so): Xpsnr, XPSNR of 4:2:0 sequences
  motion  -- ctypes binding of include/turbo_metrics_motion.h (libturbometrics_motion.so): Motion, VMAF's integer motion of a sequence
  vif     -- ctypes binding of include/turbo_metrics_vif.h (libturbometrics_vif.so): Vif, VMAF's VIF feature of frame pairs
  adm     -- ctypes binding of include/turbo_metrics_adm.h (libturbometrics_adm.so): Adm, VMAF's ADM feature of frame pairs
  scene   -- ctypes binding of include/turbo_metrics_scene.h (libturbometrics_scene.so): Scene, luma histograms and scene cuts
  cambi   -- ctypes binding of include/turbo_metrics_cambi.h (libturbometrics_cambi.so): Cambi, VMAF's banding index of one stream
  flip    -- ctypes binding of include/turbo_metrics_flip.h (libturbometrics_flip.so): Flip, the LDR-FLIP difference map of picture pairs
  yuv     -- ctypes binding of include/turbo_metrics_yuv.h (libturbometrics_yuv.so): Yuv, plane-wise PSNR and x264 / ffmpeg SSIM of 4:2:0 pairs
  hvs     -- ctypes binding of include/turbo_metrics_hvs.h (libturbometrics_hvs.so): Hvs, PSNR-HVS and PSNR-HVS-M of the lumas of frame pairs
  ciede   -- ctypes binding of include/turbo_metrics_ciede.h (libturbometrics_ciede.so): Ciede, CIEDE2000 of 4:2:0 frame pairs
  siti    -- ctypes binding of include/turbo_metrics_siti.h (libturbometrics_siti.so): Siti, ITU-T P.910 spatial / temporal information of one stream
  gmsd    -- ctypes binding of include/turbo_metrics_gmsd.h (libturbometrics_gmsd.so): Gmsd, the gradient magnitude similarity deviation of the lumas of frame pairs
  haarpsi -- ctypes binding of include/turbo_metrics_haarpsi.h (libturbometrics_haarpsi.so): HaarPsi, the Haar wavelet-based perceptual similarity index of the lumas of frame pairs
  itp     -- ctypes binding of include/turbo_metrics_itp.h (libturbometrics_itp.so): Itp, the BT.2124 colour difference dE ITP of 4:2:0 HDR (PQ / HLG) frame pairs
  mdsi    -- ctypes binding of include/turbo_metrics_mdsi.h (libturbometrics_mdsi.so): Mdsi, the mean deviation similarity index (gradient and chromaticity similarity, deviation pooling) of 4:2:0 frame pairs

There is no CPU implementation in this package: without the HIP library (or without a gfx950 GPU)
the operators raise.
"""
from . import ffi, launch, motion, shard, synth, xpsnr  # noqa: F401
from .engine import (ColorMatrix, FrameScores, HwFrame, Metrics, Ssimulacra2, TmError,  # noqa: F401
                     TurboMetrics, init_hip, set_debug_log, set_placement_candidates)
from .xpsnr import Xpsnr, XpsnrFrame  # noqa: F401,E402
from .motion import Motion, MotionFrame  # noqa: F401,E402
from . import vif  # noqa: F401,E402
from .vif import Vif, VifFrame  # noqa: F401,E402
from . import adm  # noqa: F401,E402
from .adm import Adm, AdmFrame  # noqa: F401,E402
from . import scene  # noqa: F401,E402
from .scene import Scene, SceneFrame  # noqa: F401,E402
from . import cambi  # noqa: F401,E402
from .cambi import Cambi, CambiFrame  # noqa: F401,E402
from . import flip  # noqa: F401,E402
from .flip import Flip, FlipFrame  # noqa: F401,E402
from . import yuv  # noqa: F401,E402
from .yuv import Yuv, YuvFrame  # noqa: F401,E402
from . import hvs  # noqa: F401,E402
from .hvs import Hvs, HvsFrame  # noqa: F401,E402
from . import ciede  # noqa: F401,E402
from .ciede import Ciede, CiedeFrame  # noqa: F401,E402
from . import siti  # noqa: F401,E402
from .siti import Siti, SitiFrame  # noqa: F401,E402
from . import gmsd  # noqa: F401,E402
from .gmsd import Gmsd, GmsdFrame  # noqa: F401,E402
from . import haarpsi  # noqa: F401,E402
from .haarpsi import HaarPsi, HaarPsiFrame  # noqa: F401,E402
from . import itp  # noqa: F401,E402
from .itp import Itp, ItpFrame  # noqa: F401,E402
from . import mdsi  # noqa: F401,E402
from .mdsi import Mdsi, MdsiFrame  # noqa: F401,E402
