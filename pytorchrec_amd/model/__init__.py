"""Models — mirror of ``torchrec.model`` plus the CTR models of the hot path."""
from pytorchrec_amd.model.IModel import IModel
from pytorchrec_amd.model.DeepFM import FM, DeepFM
from pytorchrec_amd.model.DCNv2 import DCNv2
from pytorchrec_amd.model.DIN import DIN
from pytorchrec_amd.model.DLRM import DLRM
from pytorchrec_amd.model.XDeepFM import XDeepFM
from pytorchrec_amd.model.AutoInt import AutoInt
from pytorchrec_amd.model.FunkSVD import FunkSVD
from pytorchrec_amd.model.SVDPP import SVDPP
from pytorchrec_amd.model.SASRec import SASRec
from pytorchrec_amd.model.GRU4Rec import GRU4Rec
from pytorchrec_amd.model.NCF import NCF
from pytorchrec_amd.model.models import get_model_type, model_name_list
