"""SURVEY §8b level 1, construction half: the reference's constructor statements must run against libvapx's classes.

CPU part (this file, ``-m "not gpu"``): the statements of ``VAPRealTime.__init__`` (vap_main.py:194-215; vap_bc_main.py:188-209 and
vap_nod_main.py:187-208 are the same lines) and of the library twin ``Vap.__init__`` (vap_realtime/model.py:25-49), restated in
``_construct_like_the_reference`` with only the class names bound to ``vap_realtime_amd.realtime``.  Nothing touches a GPU until the first
compute call, so the whole constructor runs here; what it leaves behind must pack into the bit-identical weight blob the direct path
makes.  The GPU part (tests/test_adapters_gpu.py::test_reference_constructor_lines_then_level1_orchestration) drives an object built the
same way."""
import argparse
import json
import os

import numpy as np
import pytest

from vap_realtime_amd import weights as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _write_reference_format_files(tmp_path, mode, hz=20, seed=11):
    import torch
    cpc_sd, vap_sd = W.synthetic_weights(seed, hz, mode)
    vap_t = {k: torch.from_numpy(np.asarray(v)) for k, v in vap_sd.items()}
    vap_t["encoder.encoder.gEncoder.conv0.weight"] = torch.zeros(256, 1, 10)        # real files carry encoder.* keys (ignored, vap_main.py:201)
    vap_p, cpc_p = str(tmp_path / f"{mode}_state_dict.pt"), str(tmp_path / "60k_epoch4-d0f474de.pt")
    torch.save(vap_t, vap_p)
    torch.save({"weights": {k: torch.from_numpy(np.asarray(v)) for k, v in cpc_sd.items()},
                "config": argparse.Namespace(hiddenGar=256, hiddenEncoder=256)}, cpc_p)
    return cpc_sd, vap_sd, vap_p, cpc_p


def _construct_like_the_reference(klass, sd, cpc_p, device):
    """conf -> VapGPT(conf) -> load_encoder -> load_state_dict(strict=False) -> the eight downsample assignments (weight / bias of
    downsample[1] and downsample[2].ln, on encoder1 then encoder2) -> .to(device) -> .eval(): the reference's constructor order."""
    import torch
    from vap_realtime_amd.realtime import VapConfig
    vap = klass(VapConfig())
    vap.load_encoder(cpc_model=cpc_p)
    vap.load_state_dict(sd, strict=False)
    for enc in (vap.encoder1, vap.encoder2):
        enc.downsample[1].weight = torch.nn.Parameter(sd["encoder.downsample.1.weight"])
        enc.downsample[1].bias = torch.nn.Parameter(sd["encoder.downsample.1.bias"])
        enc.downsample[2].ln.weight = torch.nn.Parameter(sd["encoder.downsample.2.ln.weight"])
        enc.downsample[2].ln.bias = torch.nn.Parameter(sd["encoder.downsample.2.ln.bias"])
    vap.to(device)
    return vap.eval()


@pytest.mark.parametrize("mode", [pytest.param("vap", id="rvap/vap_main/vap_main.py-vap"), pytest.param("bc", id="rvap/vap_bc/vap_bc_main.py-bc"),
                                  pytest.param("nod", id="rvap/vap_nod/vap_nod_main.py-nod")])
def test_reference_server_constructor_runs_verbatim(mode, tmp_path):
    """vap_main / vap_bc_main / vap_nod_main (the id names the program): each calls its class ``VapGPT`` and loads the file with
    ``torch.load``; their constructor statements, in the reference's order, through ``_construct_like_the_reference``."""
    import torch
    from vap_realtime_amd import realtime as R
    cpc_sd, vap_sd, vap_p, cpc_p = _write_reference_format_files(tmp_path, mode)
    klass = {"vap": R.VapGPT, "bc": R.VapGPT_bc, "nod": R.VapGPT_nod}[mode]
    vap = _construct_like_the_reference(klass, torch.load(vap_p, map_location=torch.device("cpu")), cpc_p, torch.device("cuda", 0))
    assert type(vap) is klass and vap.device == torch.device("cuda", 0)
    assert vap._engine is None, "nothing may touch the GPU before the first compute call"
    got_cpc, got_vap = vap._gather_state_dicts()
    assert np.array_equal(W.pack_blob(got_cpc, got_vap, mode), W.pack_blob(cpc_sd, vap_sd, mode))


@pytest.mark.parametrize("mode", ["vap", "bc", "nod"])
def test_reference_library_twin_constructor_runs_verbatim(mode, tmp_path):
    """``vap_realtime/model.py:25-49``: ``Vap.__init__`` picks VapGPT / VapGPT_bc / VapGPT_nod by ``mode``, loads through
    ``load_vap_model`` (here the local loader, checkpoints._torch_load) and moves to the device given as a string."""
    import torch
    from vap_realtime_amd import realtime as R, checkpoints
    cpc_sd, vap_sd, vap_p, cpc_p = _write_reference_format_files(tmp_path, mode)
    klass = {"vap": R.VapGPT, "bc": R.VapGPT_bc, "nod": R.VapGPT_nod}[mode]
    vap = _construct_like_the_reference(klass, checkpoints._torch_load(vap_p), cpc_p, "cuda")
    assert type(vap) is klass and vap.device == torch.device("cuda", 0) and vap._engine is None
    got_cpc, got_vap = vap._gather_state_dicts()
    assert np.array_equal(W.pack_blob(got_cpc, got_vap, mode), W.pack_blob(cpc_sd, vap_sd, mode))


def test_vapconfig_has_the_reference_fields_and_defaults():
    from vap_realtime_amd.realtime import VapConfig
    c = VapConfig()
    want = dict(sample_rate=16000, frame_hz=50, bin_times=[0.2, 0.4, 0.6, 0.8], encoder_type="cpc", wav2vec_type="mms", hubert_model="hubert_jp",
                freeze_encoder=1, load_pretrained=1, only_feature_extraction=0, dim=256, channel_layers=1, cross_layers=3, num_heads=4,
                dropout=0.1, context_limit=-1, context_limit_cpc_sec=-1, lid_classify=0, lid_classify_num_class=3,
                lid_classify_adversarial=0, lang_cond=0)                                        # vap_main.py:35-66
    assert {k: getattr(c, k) for k in c.__dataclass_fields__} == want
    with open(os.path.join(GOLDEN, "vapconfig_fields.json")) as f:                             # field-for-field against the reference's class
        assert json.load(f) == list(want) == list(c.__dataclass_fields__)                     # (tools/make_golden_config.py)
    p, added = VapConfig.add_argparse_args(argparse.ArgumentParser(), [])
    args = p.parse_args(["--vap_frame_hz", "20", "--vap_bin_times", "0.2", "0.4", "0.6", "0.8"])
    assert VapConfig.args_to_conf(args).frame_hz == 20 and added == list(want)


@pytest.mark.parametrize("field,value", [("dim", 512), ("num_heads", 8), ("channel_layers", 2), ("cross_layers", 4), ("context_limit", 100),
                                         ("encoder_type", "hubert"), ("bin_times", [0.1, 0.2, 0.3, 0.4])])
def test_unsupported_architectures_are_refused_at_construction(field, value):
    from vap_realtime_amd.realtime import VapConfig, VapGPT
    from vap_realtime_amd.engine import VapxError
    with pytest.raises(VapxError, match=field):
        VapGPT(VapConfig(**{field: value}))


def test_construction_errors_name_the_missing_reference_step(tmp_path):
    import torch
    from vap_realtime_amd.realtime import VapConfig, VapGPT, VapGPT_nod
    from vap_realtime_amd.engine import VapxError
    cpc_sd, vap_sd, vap_p, cpc_p = _write_reference_format_files(tmp_path, "vap")
    sd = torch.load(vap_p, map_location="cpu")
    m = VapGPT(VapConfig())
    with pytest.raises(VapxError, match="load_encoder"):
        m._gather_state_dicts()
    with pytest.raises(FileNotFoundError):
        m.load_encoder(cpc_model=str(tmp_path / "nope.pt"))                 # the reference would download (encoder_components.py:372-380)
    m.load_encoder(cpc_model=cpc_p)
    with pytest.raises(RuntimeError, match="Unexpected key"):              # strict=True fails on encoder.* exactly like nn.Module does
        m.load_state_dict(sd)
    res = m.load_state_dict(sd, strict=False)
    assert "encoder.downsample.1.weight" in res.unexpected_keys and "encoder1.downsample.1.weight" in res.missing_keys
    assert not [k for k in res.missing_keys if not k.startswith("encoder")]
    with pytest.raises(VapxError, match="vap_main.py:203-212"):            # the eight assignments were skipped
        m._gather_state_dicts()
    for e in (m.encoder1, m.encoder2):
        e.downsample[1].weight = torch.nn.Parameter(sd["encoder.downsample.1.weight"])
        e.downsample[1].bias = torch.nn.Parameter(sd["encoder.downsample.1.bias"])
        e.downsample[2].ln.weight = torch.nn.Parameter(sd["encoder.downsample.2.ln.weight"])
        e.downsample[2].ln.bias = torch.nn.Parameter(sd["encoder.downsample.2.ln.bias"])
    m._gather_state_dicts()
    m.encoder2.downsample[1].bias = torch.nn.Parameter(sd["encoder.downsample.1.bias"] + 1)
    with pytest.raises(VapxError, match="differ"):
        m._gather_state_dicts()
    with pytest.raises(VapxError, match="no CPU path"):
        m.to(torch.device("cpu"))
    assert "nod_head.weight" in VapGPT_nod(VapConfig()).load_state_dict(sd, strict=False).missing_keys     # a vap file into the nod class
    sd_bad = dict(sd)
    sd_bad["vap_head.weight"] = torch.zeros(128, 256)
    with pytest.raises(RuntimeError, match="size mismatch"):
        VapGPT(VapConfig()).load_state_dict(sd_bad, strict=False)
