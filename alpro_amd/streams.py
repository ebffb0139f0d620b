"""The side streams of a step: one registry (device, launch stream) -> side stream per role -- weight gradients, the text pass, the prompter's pass,
the second half batch of the no-grad forward, the precise-CLS chain (who forks, who joins, which switch governs).  What a
role keeps beside its stream are fields of its entry (a subclass of Side).  At most four streams are live at a time (profiles/r6_hw_queues.txt)."""
import contextlib

import torch

ROLES = {}     # role name -> its SideStreams


def key(device, cur=None):
    """(device index, handle of the device's current stream `cur`): what every registry is keyed by."""
    return (device.index if device.index is not None else torch.cuda.current_device(),
            cur.cuda_stream if cur is not None else torch.cuda.current_stream(device).cuda_stream)


class Side:
    """The side stream of one launch stream."""
    pending = True      # something may be queued on it that the launch stream has not waited for

    def __init__(self, stream):
        self.stream = stream

    def wait(self, cur):
        cur.wait_stream(self.stream)


class PendingSide(Side):
    """... whose user sets `pending` when it sends work there: a join with nothing pending costs no stream call."""
    pending = False

    def wait(self, cur):
        cur.wait_stream(self.stream)
        self.pending = False


class SideStreams:
    def __init__(self, role, entry=Side):
        self.role, self.entry, self.entries = role, entry, {}
        ROLES[role] = self

    def get(self, device, cur=None):
        """The entry of the current launch stream (`cur`, if the caller has it at hand), created on first use."""
        k = key(device, cur)
        ent = self.entries.get(k)
        if ent is None:
            ent = self.entries[k] = self.entry(torch.cuda.Stream(device))
        return ent

    def peek(self, device):
        """The entry of the current launch stream, or None: nothing is created."""
        return self.entries.get(key(device)) if device.type == "cuda" else None

    def owns(self, stream):
        """True if `stream` is a side stream of this role (of any launch stream)."""
        return any(e.stream.cuda_stream == stream.cuda_stream for e in self.entries.values())

    def join(self):
        """The current stream of every device waits for what this role forked from it."""
        for (idx, handle), ent in self.entries.items():
            if ent.pending:
                cur = torch.cuda.current_stream(idx)
                if cur.cuda_stream == handle:
                    ent.wait(cur)

    @contextlib.contextmanager
    def installed(self, stream, device):
        """Inside the block `stream` is this role's side stream of the current launch stream; on exit the registry is what it was before."""
        prev = dict(self.entries)
        ent = self.entries[key(device)] = self.entry(stream)
        try:
            yield ent
        finally:
            self.entries.clear()
            self.entries.update(prev)


def created_for_current(device):
    """{role: side stream} of every role that has made a side stream for the device's current launch stream."""
    k = key(device)
    return {role: reg.entries[k].stream for role, reg in ROLES.items() if k in reg.entries}


WGRAD = SideStreams("wgrad", PendingSide)   # weight-gradient GEMMs of an anchored backward (config.wgrad_side_stream)
TEXT = SideStreams("text")                  # the pretraining forward's text pass and its backward (config.text_side_stream)
PROMPTER = SideStreams("prompter")          # the frozen prompter's pass (config.prompter_side_stream)
HALF = SideStreams("half")                  # the second half batch of the no-grad encoder forward (timesformer.vit.run_blocks; "cls" is made there too)
