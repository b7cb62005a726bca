"""MI355X-native Fastformer (reference models/fastformer): the model, its dataset and its train / evaluate loops."""


def __getattr__(name):  # lazy: importing the package must not need torch or a GPU
    if name == "Fastformer":
        from .fastformer import Fastformer
        return Fastformer
    if name in ("Fastformer_wu", "StandardFastformerEncoder"):
        from . import fastformer_wu
        return getattr(fastformer_wu, name)
    if name in ("FastformerDataset", "batch_input_label_concatenation", "compute_auc_from_fixed_pos_neg_samples", "train", "evaluate"):
        from . import dataloader
        return getattr(dataloader, name)
    raise AttributeError(name)
