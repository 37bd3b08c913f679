"""Several datasets behind one index (datasets/coco_merger.py:8-35): member k covers the indices
[intervals[k-1], intervals[k]); every member is built from `{**defaults, **member.params}` and keeps its own
`augmentation` list and `input_size` (datasets.loader.DeviceLoader draws per member and refuses to batch members
of different input sizes together)."""
import logging
from importlib import import_module

import numpy as np

log = logging.getLogger(__name__)


class Dataset:
    def __init__(self, datasets, max_samples=None, **defaults):
        self.max_samples = max_samples          # accepted and unused, as in the reference
        self.datasets = {}                      # end of the member's interval -> member
        self.num_samples = 0
        for ds in datasets:
            cls = import_module('datasets.%s' % ds['name']).Dataset
            member = cls(**{**defaults, **ds['params']})
            self.num_samples += len(member)
            self.datasets[self.num_samples] = member
        self.intervals = np.array(list(self.datasets.keys()))
        log.info("merged %d datasets with a total number of %d samples", len(self.datasets), self.num_samples)

    @property
    def members(self):
        return list(self.datasets.values())

    @property
    def classes(self):
        return self.members[0].classes

    def __len__(self):
        return self.num_samples

    def locate(self, index):
        """-> (member, index inside it)"""
        if not 0 <= index < self.num_samples:
            raise IndexError("index %d outside the %d merged samples" % (index, self.num_samples))
        interval_idx = int(np.argmax(index < self.intervals))
        offset = int(self.intervals[interval_idx - 1]) if interval_idx > 0 else 0
        return self.datasets[int(self.intervals[interval_idx])], int(index) - offset

    def get(self, index, target_choice=None):
        member, local = self.locate(index)
        return member.get(local, target_choice)

    def __getitem__(self, index):
        return self.get(index)
