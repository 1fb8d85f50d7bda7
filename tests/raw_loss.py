"""What the stream and graph tests of the three fused pixel losses share (test_gpu_ldl.py, test_gpu_bbl.py,
test_gpu_bp.py): the entry point called through the C ABI with preallocated buffers, the same call on a side stream,
and the call captured into a HIP graph and replayed.  Every launch sums in a fixed order, so each comparison is
torch.equal."""
import ctypes

import torch

DEV = "cuda:0"


class RawLoss:
    """A fused loss of the C ABI with preallocated outputs and workspace, on torch's current stream.  `fn` takes
    `leading(*inputs)`, the pointers of `outputs` (in the ABI's order: the loss, the gradient, then the family's third
    output if it has one), the workspace, its size and the stream."""

    def __init__(self, fn, workspace_bytes, leading, outputs):
        self.fn, self.nb, self.leading, self.out = fn, workspace_bytes, leading, tuple(outputs)
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=DEV)
        self.loss, self.grad = self.out[:2]

    def __call__(self, *inputs):
        rc = self.fn(*self.leading(*inputs), *(t.data_ptr() for t in self.out), self.ws.data_ptr(), self.nb,
                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc

    def outputs(self):
        return tuple(t.clone() for t in self.out)


def side_stream_equals_default_stream(make, inputs):
    """The call on the default stream and again, in buffers of its own, on a side stream: every output is equal bit for
    bit.  Returns the default stream's RawLoss for what else the caller compares it with."""
    a, b = make(), make()
    a(*inputs)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b(*inputs)
    side.synchronize()
    for u, w in zip(a.outputs(), b.outputs()):
        assert torch.equal(u, w)
    return a


def replays_as_hip_graph(make, batches):
    """One eager call on batches[0], then the same call captured once and replayed after the inputs were overwritten in
    place with each batch in turn: every replay equals the eager result for the batch then in the buffers, bit for bit
    (the pattern of test_gpu_tiny.py::test_tiny_step_replays_as_hip_graph).  Returns the last batch's outputs."""
    bufs = tuple(t.clone() for t in batches[0])
    eager, rec = make(), make()
    eager(*bufs)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rec(*bufs)
    for batch in batches:
        for dst, src in zip(bufs, batch):
            dst.copy_(src)
        eager(*bufs)
        torch.cuda.synchronize()
        want = eager.outputs()
        for t in rec.out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for u, w in zip(rec.outputs(), want):
            assert torch.equal(u, w)
    return want
