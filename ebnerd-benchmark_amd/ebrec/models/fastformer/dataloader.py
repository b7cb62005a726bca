"""FastformerDataset and train / evaluate loops with the signatures and the observable behaviour of the reference's
models/fastformer/dataloader.py, over the pandas frames this package uses instead of polars.  Torch does the loss and the optimizer;
the model's forward / backward are HIP launches.  The loops are built from three small helpers: a sample-weighted running mean, a
tracker of the monitored validation metric (checkpoint on improvement, patience), and an optional TensorBoard scalar writer."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn
import torch.optim as optim
from functools import partial
from torch.utils.data import DataLoader, Dataset

from ebrec.evaluation import AucScore
from ebrec.models.newsrec.dataloader import _map_ids
from ebrec.utils._constants import DEFAULT_INVIEW_ARTICLES_COL, DEFAULT_LABELS_COL
from ebrec.utils._frames import list_column, to_pandas
from ebrec.utils._python import convert_to_nested_list, create_lookup_objects, repeat_by_list_values_from_matrix
from ebrec.utils._torch import save_checkpoint


def _shuffle_rows(df, seed=None):
    return df.sample(frac=1.0, random_state=seed).reset_index(drop=True)


def _rows(cells, mapping):
    """The cells of a list column as lists of lookup-matrix rows (unknown / null ids -> row 0)."""
    flat, off = _map_ids(cells, mapping)
    return [flat[off[i]:off[i + 1]] for i in range(len(off) - 1)]


@dataclass(eq=False)
class FastformerDataset(Dataset):
    """One item is a whole mini-batch of `batch_size` impressions, every in-view article unfolded into its own (history, candidate)
    pair: use ``DataLoader(dataset)`` with the DataLoader's own batch_size = 1 (the output is then (1, *shape)) and
    ``batch_input_label_concatenation`` to drop that axis, as the reference does."""

    behaviors: object
    history_column: str
    article_dict: dict
    batch_size: int = 64
    shuffle: bool = True
    device: str = "cpu"
    seed: int = None
    labels_col: str = DEFAULT_LABELS_COL
    inview_col: str = DEFAULT_INVIEW_ARTICLES_COL
    n_samples_col: str = "n_samples"

    def __post_init__(self):
        self.unknown_index = [0]
        self.behaviors = to_pandas(self.behaviors).reset_index(drop=True)
        if self.shuffle:
            self.behaviors = _shuffle_rows(self.behaviors, seed=self.seed)
        self.behaviors[self.n_samples_col] = [len(l) for l in list_column(self.behaviors, self.labels_col)]
        self.lookup_indexes, self.lookup_matrix = create_lookup_objects(self.article_dict, unknown_representation="zeros")

    def __len__(self):
        """Number of batch steps in the data."""
        return int(np.ceil(self.behaviors.shape[0] / self.batch_size))

    def __getitem__(self, index: int):
        batch = self.behaviors.iloc[index * self.batch_size:(index + 1) * self.batch_size]
        if len(batch) == 0:
            raise IndexError(index)
        if self.shuffle:
            batch = _shuffle_rows(batch, seed=self.seed)
        his = _rows(batch[self.history_column].tolist(), self.lookup_indexes)
        inv = _rows(batch[self.inview_col].tolist(), self.lookup_indexes)
        repeats = np.array(batch[self.n_samples_col])
        history_input = repeat_by_list_values_from_matrix(input_array=np.stack(his), matrix=self.lookup_matrix, repeats=repeats)
        candidate_input = self.lookup_matrix[np.concatenate(inv)][:, None, :]
        labels = np.concatenate([np.asarray(l, dtype=np.float32) for l in list_column(batch, self.labels_col)])
        history_input = torch.as_tensor(history_input).type(torch.int).to(self.device)
        candidate_input = torch.as_tensor(candidate_input).type(torch.int).to(self.device)
        y = torch.as_tensor(labels).view(-1, 1).type(torch.float).to(self.device)
        return (history_input, candidate_input), y


def batch_input_label_concatenation(inputs, labels):
    """The DataLoader adds a leading axis of 1 to the dataset's ready-made batch: drop it from both inputs and the labels."""
    history, candidates = (t.squeeze(0) for t in inputs)
    return (history, candidates), labels.squeeze(0)


def compute_auc_from_fixed_pos_neg_samples(y_true, y_pred) -> float:
    """Validation AUC as the reference computes it: the flat label / score lists are cut into consecutive groups of
    ``int(sum(y_true))`` elements (one positive per impression and equal in-view lengths make every group well defined) and the
    AUC is averaged over the groups."""
    groups = partial(convert_to_nested_list, sublist_size=int(np.sum(y_true)))
    return AucScore().calculate(y_true=groups(y_true), y_pred=groups(y_pred))


class _RunningMean:
    """Sample-weighted mean of per-batch means."""

    def __init__(self):
        self.total, self.count = 0.0, 0

    def add(self, batch_mean: float, n: int) -> float:
        self.total += batch_mean * n
        self.count += n
        return self.value

    @property
    def value(self) -> float:
        return self.total / self.count


class _Monitor:
    """Follows the monitored validation metric: `improved` says when to checkpoint, `out_of_patience` when to stop."""

    SIGN = {"loss": -1.0, "auc": 1.0}  # larger sign * value is better

    def __init__(self, metric: str, patience):
        if metric not in self.SIGN:
            raise ValueError(f"monitor_metric = {metric!r}: one of {sorted(self.SIGN)}")
        self.metric, self.patience = metric, patience
        self.best, self.stale = -np.inf, 0

    def improved(self, value: float) -> bool:
        merit = self.SIGN[self.metric] * value
        if merit > self.best:
            self.best, self.stale = merit, 0
            return True
        self.stale += 1
        return False

    @property
    def out_of_patience(self) -> bool:
        return self.patience is not None and self.stale == self.patience


class _Scalars:
    """add_scalar on an optional SummaryWriter (anything with add_scalar / close)."""

    def __init__(self, writer):
        self.writer = writer

    def __call__(self, tag: str, value: float, step: int):
        if self.writer is not None:
            self.writer.add_scalar(tag=tag, scalar_value=value, global_step=step)

    def close(self):
        if self.writer is not None:
            self.writer.close()


def _progress(loader, title: str, disable: bool, ncols: int):
    from tqdm import tqdm

    return tqdm(loader, desc=title, total=len(loader), disable=disable, ncols=ncols)


def train(model: nn.Module, train_dataloader: DataLoader, criterion: nn.Module, optimizer: optim.Optimizer, num_epochs: int = 5,
          val_dataloader: DataLoader = None, state_dict_path: str = "model_state_dict.pt", patience: int = None, summary_writer=None,
          gradient_accumulation_steps: int = 1, tqdm_disable: bool = False, tqdm_ncol: int = 80, monitor_metric: str = "loss") -> nn.Module:
    """Train for up to `num_epochs`.  Gradients accumulate over `gradient_accumulation_steps` batches (and are applied at the last
    batch of an epoch whatever its index).  With a `val_dataloader`, every epoch ends in an evaluation: the state is saved to
    `state_dict_path` whenever `monitor_metric` ("loss" or "auc") improves, training stops after `patience` epochs without
    improvement, and the best saved state is loaded back before the model is returned.  The reported training loss is the running
    mean over every sample seen so far, across epochs."""
    monitor = _Monitor(monitor_metric, patience)
    scalars = _Scalars(summary_writer)
    seen = _RunningMean()
    step, last = 0, len(train_dataloader)
    for epoch in range(1, num_epochs + 1):
        model.train()
        optimizer.zero_grad()
        bar = _progress(train_dataloader, f"Epoch [{epoch}/{num_epochs}]", tqdm_disable, tqdm_ncol)
        for index, packed in enumerate(bar, start=1):
            (history, candidates), target = batch_input_label_concatenation(*packed)
            scores = model(history, candidates)
            loss = criterion(scores, target)
            loss.backward()
            step += 1
            mean = seen.add(loss.item(), len(scores))
            bar.set_postfix({"Loss": round(mean, 6)})
            scalars("Train/Loss", mean, step)
            if index % gradient_accumulation_steps == 0 or index == last:
                optimizer.step()
                optimizer.zero_grad()
        if not val_dataloader:
            continue
        val_scores, val_labels, val_loss = evaluate(model, val_dataloader, criterion, tqdm_disable=tqdm_disable)
        scalars("Val/Loss", val_loss, step)
        watched = val_loss
        if monitor.metric == "auc":
            watched = compute_auc_from_fixed_pos_neg_samples(y_true=np.ravel(val_labels.tolist()), y_pred=np.ravel(val_scores.tolist()))
            print(f"Val/AUC : {watched:.6f}")
            scalars("Val/AUC", watched, step)
        if monitor.improved(watched):
            save_checkpoint(model, path=state_dict_path)
        if monitor.out_of_patience:
            break
    scalars.close()
    if val_dataloader:
        model.load_state_dict(torch.load(state_dict_path), strict=True)
    return model


def evaluate(model: nn.Module, dataloader: DataLoader, criterion: nn.Module, tqdm_disable: bool = False, tqdm_ncol: int = 80,
             device: str = "cpu"):
    """-> (scores [n, 1], labels [n, 1], sample-weighted mean loss) over the loader, in eval mode and without gradients.  `device`
    is accepted for signature compatibility; the tensors stay where the loader put them."""
    model.eval()
    mean = _RunningMean()
    scores_seen, labels_seen = [], []
    bar = _progress(dataloader, "Evaluating", tqdm_disable, tqdm_ncol)
    with torch.no_grad():
        for packed in bar:
            (history, candidates), target = batch_input_label_concatenation(*packed)
            scores = model(history, candidates)
            bar.set_postfix({"Eval Loss": round(mean.add(criterion(scores, target).item(), len(scores)), 4)})
            scores_seen.append(scores)
            labels_seen.append(target)
    return torch.cat(scores_seen, dim=0), torch.cat(labels_seen, dim=0), mean.value
