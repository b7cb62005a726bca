"""MI355X-native NRMS / NRMSDocVec, NPA and LSTUR (user-id models), and NAML (multi-view news encoder)."""
from .model_config import hparams_lstur, hparams_naml, hparams_npa, hparams_nrms, hparams_nrms_docvec, hparams_to_dict, print_hparams  # noqa: F401


def __getattr__(name):  # lazy: importing model_config / dataloader must not need torch or a GPU
    if name == "NRMSModel":
        from .nrms import NRMSModel
        return NRMSModel
    if name == "NRMSDocVec":
        from .nrms_docvec import NRMSDocVec
        return NRMSDocVec
    if name == "NPAModel":
        from .npa import NPAModel
        return NPAModel
    if name == "LSTURModel":
        from .lstur import LSTURModel
        return LSTURModel
    if name == "NAMLModel":
        from .naml import NAMLModel
        return NAMLModel
    raise AttributeError(name)
