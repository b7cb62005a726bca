"""Torch helpers (the counterpart of the reference's utils/_torch.py)."""
import os
from pathlib import Path


def save_checkpoint(model, path="model_state_dict.pt"):
    """Write ``model.state_dict()`` to `path` (its directory is created when missing) and return the path written."""
    import torch

    target = Path(path)
    os.makedirs(target.parent, exist_ok=True)
    torch.save(model.state_dict(), str(target))
    print(f"model weights saved to {target}")
    return target
