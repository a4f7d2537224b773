"""Where the one-kernel conv2_1 / conv2_2 route applies (Network._conv2_fused_at, posecnn_amd/networks.py), without a GPU: with
the default block minimum the small graphs of the route tables stay on the unfused pair, the 16-frame RGB-D step takes it."""
import torch

from posecnn_amd.networks import Network, vgg16_convs


def _net(fmt):
    return vgg16_convs(fmt, 22, 64, (1.0,), 1.0, -1.0, vertex_reg_2d=True, pose_reg=True, trainable=False, is_train=False,
                       seed=3, init="he", with_losses=False, device="cpu")


def test_default_minimum_keeps_small_graphs_unfused_and_takes_the_flagship():
    assert Network.fused_conv2 is True and Network.fused_conv2_min_blocks >= 49      # class attributes, no new __init__ flag
    net = _net("RGBD")
    assert "fused_conv2" not in vars(net) and "fused_conv2_min_blocks" not in vars(net)
    with torch.no_grad():
        for B in (1, 2):
            for H, W in ((32, 48), (96, 128)):
                for towers in (1, 2):   # layer by layer, and the two towers stacked
                    for cin in (64, 128):
                        assert not net._conv2_fused_at(towers * B, H // 2, W // 2, cin, 128), (B, H, W, towers, cin)
                assert not net._conv2_layers_fused(B, H, W)
        assert net._conv2_fused_at(32, 240, 320, 64, 128) and net._conv2_fused_at(32, 240, 320, 128, 128)
        assert net._conv2_layers_fused(16, 480, 640)
        # everything else the predicate asks for
        assert not net._conv2_fused_at(32, 240, 320, 128, 256) and not net._conv2_fused_at(32, 240, 320, 256, 128)
        assert not net._conv2_fused_at(32, 232, 320, 64, 128) and not net._conv2_fused_at(32, 240, 328, 64, 128)
        for flag, off in (("fused_conv2", False), ("winograd_mfma", False), ("winograd_packed", False), ("winograd_tile", 2)):
            setattr(net, flag, off)
            assert not net._conv2_fused_at(32, 240, 320, 64, 128), flag
            if flag in ("fused_conv2", "winograd_packed"):
                delattr(net, flag)
            else:
                setattr(net, flag, True if flag == "winograd_mfma" else 4)
        assert net._conv2_fused_at(32, 240, 320, 64, 128)
        net.fused_conv2_min_blocks = 1   # counts as the floor: below it the unfused conv2_2 splits Cin, other bits
        assert not net._conv2_fused_at(1, 16, 16, 64, 128) and not net._conv2_fused_at(127, 16, 16, 128, 128)
        assert net._conv2_fused_at(128, 16, 16, 128, 128)
        net.fused_conv2_min_blocks = 1000
        assert not net._conv2_fused_at(999, 16, 16, 64, 128) and net._conv2_fused_at(1000, 16, 16, 64, 128)


def test_tables_move_the_two_layers_to_the_new_kernel():
    net = _net("RGBD")
    with torch.no_grad():
        on_f, on_b = net.mfma_table(16, 480, 640), net.hbm_table(16, 480, 640)
        net.fused_conv2 = False
        off_f, off_b = net.mfma_table(16, 480, 640), net.hbm_table(16, 480, 640)
    assert "conv2_wino43_fused_kernel" not in off_f and "conv2_wino43_fused_kernel" not in off_b
    tiles = 16 * 60 * 80
    fl = 2 * 2.0 * 36 * tiles * (64 + 128) * 128
    assert on_f["conv2_wino43_fused_kernel"] == fl and off_f["wino43_mfma_kernel"] - on_f["wino43_mfma_kernel"] == fl
    assert sum(on_f.values()) == sum(off_f.values())
    act = lambda div, ch: 4.0 * 16 * (480 // div) * (640 // div) * ch
    assert off_b["wino43_input_kernel"] - on_b["wino43_input_kernel"] == 2 * 3.25 * (act(2, 64) + act(2, 128))
    assert on_b["conv2_wino43_fused_kernel"] == 2 * (act(2, 64) + 2 * act(2, 128) + act(4, 128))
