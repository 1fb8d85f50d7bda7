"""ssl_amd/_gpu.py, the one way a C-ABI call reaches the GPU, as far as it can be held without one: what `launch` hands
to the entry point and does with its status, what `on` and `stream` are for a device that is no GPU, and that no other
module of the package spells a stream handle or a `_launch` of its own."""
import ast
import contextlib
import glob
import os

import pytest
import torch

PACKAGE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ssl_amd")
CPU = torch.device("cpu")


def _recording(status):
    calls = []

    def fake(*args):
        calls.append(args)
        return status
    return fake, calls


def test_launch_appends_the_stream_and_checks_the_status():
    from ssl_amd import _gpu, _lib
    fake, calls = _recording(0)
    assert _gpu.launch(CPU, fake, 1, 2) is None
    assert calls == [(1, 2, None)]
    fake, calls = _recording(-1)
    with pytest.raises(RuntimeError) as err:
        _gpu.launch(CPU, fake, 1, 2)
    assert calls == [(1, 2, None)]
    assert _lib.lib().ssg_status_string(-1).decode() in str(err.value) and "(status -1)" in str(err.value)


def test_a_device_that_is_no_gpu_needs_no_context_and_has_no_stream():
    from ssl_amd import _gpu
    assert isinstance(_gpu.on(CPU), contextlib.nullcontext)
    with _gpu.on(CPU) as entered:
        assert entered is None
    assert _gpu.stream(CPU) is None
    assert _gpu.ptr(None) is None and _gpu.ptr(torch.zeros(1)) != 0
    with pytest.raises(RuntimeError, match="expected a GPU tensor, got device cpu"):
        _gpu.need_gpu(None, torch.zeros(1))


def test_the_engines_names_are_the_leaf_modules():
    from ssl_amd import _gpu, engine
    for name, target in (("_ptr", _gpu.ptr), ("_stream", _gpu.stream), ("_launch", _gpu.launch), ("_need_gpu", _gpu.need_gpu),
                         ("_workspace", _gpu.workspace), ("address_array", _gpu.address_array),
                         ("dense_strides", _gpu.dense_strides)):
        assert getattr(engine, name) is target, name


def test_one_spelling():
    """Only _gpu.py reads a stream's handle, and only engine.py and _gpu.py may define a function named `_launch`."""
    paths = sorted(glob.glob(os.path.join(PACKAGE, "**", "*.py"), recursive=True))
    assert len(paths) > 20 and os.path.join(PACKAGE, "_gpu.py") in paths
    for path in paths:
        name = os.path.relpath(path, PACKAGE)
        if name == "_gpu.py":
            continue
        with open(path) as f:
            text = f.read()
        for word in (".cuda_stream", "_cuda_getCurrentRawStream"):
            assert word not in text, f"{name} spells {word}"
        if name != "engine.py":
            defined = [n.name for n in ast.walk(ast.parse(text)) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]
            assert "_launch" not in defined, f"{name} defines a _launch of its own"


def test_the_leaf_module_imports_nothing_else_of_the_package():
    with open(os.path.join(PACKAGE, "_gpu.py")) as f:
        tree = ast.parse(f.read())
    relative = [(n.module, [a.name for a in n.names]) for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.level]
    assert relative == [(None, ["_lib"])]
