"""CPU: the small nature CNN's configs load through the registry, and the input-layer family table keeps answering by plane
count alone as before it learned the filter count."""
from rltime_amd.general.config import load_config, validate_config


def test_small_cnn_configs_load():
    module = load_config("models/modules/nature_cnn_small.json")
    assert module["type"] == "cnn" and module["args"]["channels_last"] is True
    assert [(s["filters"], s["kernel"], s["stride"]) for s in module["args"]["layers"]] == [(16, 8, 4), (32, 4, 2)]
    cfg = load_config("catch_dqn_small.json")
    validate_config({k: v for k, v in cfg.items() if k != "_comment"})
    assert cfg["model"]["args"]["layer_configs"][0] == module
    base = load_config("catch_dqn.json")
    assert {k: v for k, v in cfg.items() if k not in ("_comment", "model")} == {k: v for k, v in base.items() if k not in ("_comment", "model")}
    assert cfg["env_args"]["frame_shape"] == [4, 84, 84]                 # both layers accept it: 84 -> 20 -> 9


def test_family_table_by_planes_and_filters():
    from rltime_amd.models.torch import fused
    for planes in (1, 3, 4):
        assert fused.conv_u8_family(planes) is fused._CONV_U8[planes] is fused.conv_u8_family(planes, 32)
        small = fused.conv_u8_family(planes, 16)
        assert small.planes == planes and small is not fused.conv_u8_family(planes) and small.prefix.startswith("mirl_conv1f16p")
        assert small.supported(84, 84, 16, 8, 4) and not small.supported(84, 84, 32, 8, 4)      # host logic: no GPU needed
    assert fused.conv_u8_family(2) is None and fused.conv_u8_family(2, 16) is None and fused.conv_u8_family(4, 64) is None
