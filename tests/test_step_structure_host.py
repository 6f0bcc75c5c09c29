"""CPU: the host layer that sequences a step states each shared piece once -- the energy-and-force chain, the recorder, the
driver loop, the kept buffers' properties and the periodic-argument refusals.  Needs no library."""
import glob
import os


def _source(repo_root, *names):
    return {n: open(os.path.join(repo_root, "gotennet_amd", n)).read() for n in names}


def test_one_chain_one_recorder_one_loop(repo_root):
    from gotennet_amd import md, pipeline, relax
    src = _source(repo_root, "pipeline.py", "md.py", "relax.py")
    # the chain: forward -> head -> backward -> force scatter [-> virial], in pipeline.energy_forces and nowhere else
    assert src["pipeline.py"].count("engine.backward(") == 1
    assert "engine.backward(" not in src["md.py"] and "engine.backward(" not in src["relax.py"]
    assert callable(pipeline.energy_forces)
    # the recorder: one side-stream warm-up and one capture in the package
    package = {p: open(p).read() for p in glob.glob(os.path.join(repo_root, "gotennet_amd", "**", "*.py"), recursive=True)}
    assert sum(s.count("CUDAGraph(") for s in package.values()) == 1
    # the loop: no second copy for the device-rebuilt list; the eager step borrows nothing
    assert not hasattr(md._ListDriver, "_run_device")
    assert getattr(md._EagerStep, "_body", None) is not pipeline.CapturedStep._body
    assert "run" not in vars(md.MDRun) and issubclass(relax.Relax, md._ListDriver)
    # the kept buffers' properties: the base's, inherited by both drivers
    for name in ("pos", "vel", "potential_energy", "stress"):
        assert isinstance(vars(md._ListDriver)[name], property), name
        assert name not in vars(md.MDRun) and name not in vars(relax.Relax), name
        assert isinstance(getattr(relax.Relax, name), property) and isinstance(getattr(md.MDRun, name), property)
    # whether the cell moves is the driver's to say, not the step's to find out
    assert md._ListDriver._cell_moves is False and "getattr(md" not in src["md.py"]
    # the periodic-argument refusals: each message once in the package
    everything = "".join(package.values())
    assert everything.count('cell requires grad: autograd with respect to the cell is not supported")') == 1
    assert everything.count("images must be one of") == 1
