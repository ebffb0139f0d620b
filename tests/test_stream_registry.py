"""The two things the stream schedule of a step is made of: the runtime switches of alpro_amd.config -- one type, one table,
one override context -- and the side-stream registry of alpro_amd.streams.  The switch tests need no device; the registry test launches nothing."""
import pytest
import torch

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
SPLIT_B = (1, 2, 3, 15, 16, 17, 64)
AUTO_B, ON_B, OFF_B = [False, False, False, False, True, False, True], [False, True, False, False, True, False, True], [False] * 7

# switch -> (decision, its argument sets, [(value given to set_*, value held afterwards, the decision per argument set)]): what the functions gave
# before the switches shared a type, written down once
TABLE = {
    "split_streams": ("split_streams", [(b,) for b in SPLIT_B], [
        ("auto", "auto", AUTO_B), ("1", "1", ON_B), ("0", "0", OFF_B), (True, "1", ON_B), (False, "0", OFF_B), ("ON", "on", ON_B), ("Off", "off", OFF_B),
        ("true", "true", ON_B), ("infer", "infer", AUTO_B), ("banana", "banana", AUTO_B)]),
    "cls_stream": ("cls_stream", [(False,), (True,)], [
        ("infer", "infer", [True, False]), ("1", "1", [True, True]), ("0", "0", [False, False]), (True, "1", [True, True]), (False, "0", [False, False]),
        ("On", "on", [True, True]), ("auto", "auto", [False, False])]),
    "fuse_temporal_attention": ("fuse_temporal_attention", [(False,), (True,)], [
        ("infer", "infer", [True, False]), ("1", "1", [True, True]), ("0", "0", [False, False]), (True, "1", [True, True]), (False, "0", [False, False]),
        ("On", "on", [True, True]), ("auto", "auto", [False, False])]),
    "cls_precise": ("cls_precise", [(F16,), (BF16,), (F32,)], [
        ("auto", "auto", [True, False, False]), ("1", "1", [True, True, False]), ("0", "0", [False, False, False]), (True, "1", [True, True, False]),
        (False, "0", [False, False, False]), ("TRUE", "true", [True, True, False]), ("infer", "infer", [False, False, False])]),
}
ON_OFF = [(True, True, [True]), (False, False, [False]), (0, False, [False]), (1, True, [True]), ("0", True, [True]), ("", False, [False])]
for _name, _fn in (("wgrad_stream", "wgrad_stream_enabled"), ("text_stream", "text_stream_enabled"), ("prompter_stream", "prompter_stream_enabled"),
                   ("defer_temporal_add", "defer_temporal_add"), ("recompute", "recompute_blocks")):
    TABLE[_name] = (_fn, [()], ON_OFF)

# switch -> (environment variable, [(its text, value held)]); None: the variable is not set
ENV = {
    "cls_precise": ("ALPRO_CLS_PRECISE", [(None, "auto"), ("AUTO", "auto"), ("1", "1")]),
    "cls_stream": ("ALPRO_CLS_STREAM", [(None, "infer"), ("Infer", "infer"), ("0", "0")]),
    "fuse_temporal_attention": ("ALPRO_FUSE_TATTN", [(None, "infer"), ("1", "1")]),
    "split_streams": ("ALPRO_SPLIT_STREAMS", [(None, "auto"), ("OFF", "off"), ("1", "1")]),
    "wgrad_stream": ("ALPRO_WGRAD_STREAM", [(None, True), ("0", False), ("1", True), ("force", True)]),
    "text_stream": ("ALPRO_TEXT_STREAM", [(None, True), ("0", False), ("1", True)]),
    "prompter_stream": ("ALPRO_PROMPTER_STREAM", [(None, True), ("0", False), ("force", True)]),
    "defer_temporal_add": ("ALPRO_DEFER_TEMPORAL_ADD", [(None, True), ("0", False), ("false", True)]),
    "recompute": ("ALPRO_RECOMPUTE", [(None, False), ("0", False), ("1", True), (" 1 ", True)]),
}


def test_every_switch_decides_as_before(monkeypatch):
    from alpro_amd import config as rt
    assert set(rt.SWITCHES) == set(TABLE) == set(ENV)
    for name, (fn, argsets, rows) in TABLE.items():
        sw, decide, setter = rt.SWITCHES[name], getattr(rt, fn), getattr(rt, "set_" + name)
        with rt.override(name):
            for given, held, want in rows:
                setter(given)
                assert sw[0] == held and type(sw[0]) is type(held), (name, given, sw[0])
                assert [decide(*a) for a in argsets] == want, (name, given)
                setter(sw[0])                                    # what [0] yields is accepted and restores exactly
                assert sw[0] == held and [decide(*a) for a in argsets] == want, (name, given)
            env, texts = ENV[name]
            assert sw.env == env
            for text, held in texts:
                if text is None:
                    monkeypatch.delenv(env, raising=False)
                else:
                    monkeypatch.setenv(env, text)
                sw.read_env()
                assert sw[0] == held and type(sw[0]) is type(held), (name, text, sw[0])
    # the keyword forms the model code uses, and cls_precise's default argument (the compute dtype) and its off-scope
    with rt.override(cls_stream="infer", fuse_temporal_attention="infer", cls_precise="auto"):
        assert rt.cls_stream() and not rt.cls_stream(training=True) and rt.fuse_temporal_attention() and not rt.fuse_temporal_attention(training=True)
        with rt.use_compute_dtype("fp16"):
            assert rt.cls_precise() is True
            with rt.cls_precise_off():
                assert rt.cls_precise() is False
        with rt.use_compute_dtype("bf16"):
            assert rt.cls_precise() is False


def test_override_nests_and_restores_exactly_what_was_set():
    from alpro_amd import config as rt
    split, precise = rt.SWITCHES["split_streams"], rt.SWITCHES["cls_precise"]
    with rt.override("split_streams", "wgrad_stream", "cls_precise"):
        rt.set_split_streams("auto")
        rt.set_wgrad_stream(True)
        rt.set_cls_precise("1")
        with rt.override(split_streams="0", wgrad_stream=False):
            assert split[0] == "0" and not rt.split_streams(64) and rt.wgrad_stream_enabled() is False
            with rt.override("wgrad_stream", split_streams=True):
                assert split[0] == "1" and rt.split_streams(2)
                rt.set_wgrad_stream(True)                        # a switch that is only named: the block sets it, the exit puts it back
                assert rt.wgrad_stream_enabled() is True
                with rt.use_cls_precise(False), rt.use_recompute(True):
                    assert precise[0] == "0" and rt.recompute_blocks() is True
                assert precise[0] == "1"
            assert split[0] == "0" and rt.wgrad_stream_enabled() is False
        assert split[0] == "auto" and rt.split_streams(16) and not rt.split_streams(2)      # "auto" comes back as "auto"
        assert rt.wgrad_stream_enabled() is True
        with pytest.raises(KeyError, match="inside"):
            with rt.override(split_streams="1", text_stream=not rt.text_stream_enabled()):
                raise KeyError("inside")
        assert split[0] == "auto"
        text = rt.text_stream_enabled()
        with pytest.raises(KeyError, match="no_such_switch"):
            with rt.override(text_stream=not text, no_such_switch=1):
                pass
        assert rt.text_stream_enabled() is text                  # an unknown name is refused before anything is set


@pytest.mark.parametrize("value", ["yes", "2", ""])
def test_a_bad_recompute_value_raises_the_message(monkeypatch, value):
    from alpro_amd import config as rt
    monkeypatch.setenv("ALPRO_RECOMPUTE", value)
    with rt.override("recompute"):
        with pytest.raises(ValueError) as e:
            rt.SWITCHES["recompute"].read_env()
    assert str(e.value) == "ALPRO_RECOMPUTE=%r: expected 0 (keep every ViT block activation, the default) or 1 (recompute them in backward)" % value.strip()


@pytest.mark.gpu
def test_registry_keeps_one_side_stream_per_role_and_launch_stream(monkeypatch):
    from alpro_amd import streams
    from alpro_amd.modeling.timesformer import vit  # noqa: F401  (the fifth role, "cls", is made beside its entry type)
    assert sorted(streams.ROLES) == ["cls", "half", "prompter", "text", "wgrad"]
    for reg in streams.ROLES.values():      # empty registries for this test: torch hands out stream handles from a pool of 32 in turn, so the streams
        monkeypatch.setattr(reg, "entries", {})   # made below are distinct handles, which those made over a whole session need not be
    dev = torch.device("cuda", torch.cuda.current_device())
    main, other = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
    mine = {role: reg.get(dev).stream for role, reg in streams.ROLES.items()}
    for role, reg in streams.ROLES.items():
        assert reg.get(dev).stream is mine[role] and reg.peek(dev).stream is mine[role]                  # the same launch stream twice
        assert reg.get(torch.device("cuda")).stream is mine[role]                                         # ... also named without its index
        assert reg.peek(torch.device("cpu")) is None
    handles = {s.cuda_stream for s in mine.values()}
    assert len(handles) == 5 and main.cuda_stream not in handles and other.cuda_stream not in handles
    assert streams.created_for_current(dev) == mine
    with torch.cuda.stream(other):                                                                       # a second launch stream
        for role in ("cls", "half"):
            assert role not in streams.created_for_current(dev) and streams.ROLES[role].peek(dev) is None
        theirs = {role: streams.ROLES[role].get(dev).stream for role in ("cls", "half")}
        assert streams.created_for_current(dev)["half"] is theirs["half"]
    assert handles.isdisjoint(s.cuda_stream for s in theirs.values()) and theirs["cls"].cuda_stream != theirs["half"].cuda_stream
    assert streams.ROLES["half"].get(dev).stream is mine["half"]
    for role, reg in streams.ROLES.items():                                                               # owns: the role that made the stream, no other
        assert [r for r in streams.ROLES if reg.owns(streams.ROLES[r].get(dev).stream)] == [role]
        assert not reg.owns(main) and not reg.owns(other)
    assert streams.ROLES["half"].owns(theirs["half"]) and not streams.ROLES["cls"].owns(theirs["half"])
    # the install hook: the given stream for this launch stream, the previous one back on exit (also after an exception, also when there was none)
    given = torch.cuda.Stream(dev)
    with streams.TEXT.installed(given, dev) as ent:
        assert streams.TEXT.get(dev) is ent and ent.stream is given and streams.TEXT.owns(given) and not streams.TEXT.owns(mine["text"])
        with pytest.raises(KeyError):
            with streams.WGRAD.installed(given, dev) as went:
                assert went.pending is False and streams.WGRAD.peek(dev) is went
                raise KeyError("inside")
        assert streams.WGRAD.get(dev).stream is mine["wgrad"]
    assert streams.TEXT.get(dev).stream is mine["text"] and not streams.TEXT.owns(given)
    with torch.cuda.stream(other):
        with streams.TEXT.installed(given, dev):
            assert streams.TEXT.peek(dev).stream is given
        assert streams.TEXT.peek(dev) is None
    # join with nothing sent: the weight-gradient entry stays clear and nothing raises
    streams.WGRAD.join()
    streams.TEXT.join()
    assert streams.WGRAD.peek(dev).pending is False
    torch.cuda.synchronize()
