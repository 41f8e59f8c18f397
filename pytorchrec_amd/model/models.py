"""Model registry — mirror of torchrec/model/models.py:8-30 (the plug-in point)."""
from typing import Dict, Type

from pytorchrec_amd.model.DCNv2 import DCNv2
from pytorchrec_amd.model.DeepFM import FM, DeepFM
from pytorchrec_amd.model.DIN import DIN
from pytorchrec_amd.model.DLRM import DLRM
from pytorchrec_amd.model.FunkSVD import FunkSVD
from pytorchrec_amd.model.GRU4Rec import GRU4Rec
from pytorchrec_amd.model.IModel import IModel
from pytorchrec_amd.model.NCF import NCF
from pytorchrec_amd.model.SASRec import SASRec
from pytorchrec_amd.model.SVDPP import SVDPP
from pytorchrec_amd.model.XDeepFM import XDeepFM
from pytorchrec_amd.model.AutoInt import AutoInt

_model_classes: Dict[str, Type[IModel]] = {
    "funksvd": FunkSVD,
    "svdpp": SVDPP,
    "sasrec": SASRec,
    "gru4rec": GRU4Rec,
    "ncf": NCF,
    "fm": FM,
    "deepfm": DeepFM,
    "dcnv2": DCNv2,
    "din": DIN,
    "dlrm": DLRM,
    "xdeepfm": XDeepFM,
    "autoint": AutoInt,
}

model_name_list = _model_classes.keys()


def get_model_type(model_name: str) -> Type[IModel]:
    if (not isinstance(model_name, str)) or (model_name not in _model_classes):
        raise ValueError(f"model_name参数不合法: {model_name}")
    return _model_classes[model_name]
