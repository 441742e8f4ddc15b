"""The recommenders of `openrec.tf2.recommenders` (same class names, constructor arguments and call signatures),
each running its train step as a fused device call: see the file of the same name."""
from . import bpr as _bpr, dlrm as _dlrm, gmf as _gmf, lightgcn as _lightgcn, mult_dae as _mdae, ucml as _ucml, vanilla_youtube_rec as _vyr, vbpr as _vbpr, wrmf as _wrmf, youtube_rec as _ytr

BPR, UCML, GMF, WRMF, DLRM = _bpr.BPR, _ucml.UCML, _gmf.GMF, _wrmf.WRMF, _dlrm.DLRM
LightGCN = _lightgcn.LightGCN
VBPR = _vbpr.VBPR
VanillaYouTubeRec = _vyr.VanillaYouTubeRec
YouTubeRec = _ytr.YouTubeRec
MultDAE = _mdae.MultDAE

__all__ = ["BPR", "UCML", "GMF", "WRMF", "DLRM", "LightGCN", "VBPR", "VanillaYouTubeRec", "YouTubeRec", "MultDAE"]
