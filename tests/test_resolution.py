"""Batch sizing by resolution (engine.batch_for_free_hbm, generate_data.auto_engine_batch): the host-side part of running 384 / 640 /
768-pixel images.  No GPU needed."""
import pytest

GB = 10 ** 9
SWEEP = [g * GB for g in range(0, 301)]
LATENTS = (16, 32, 48, 64, 80, 96, 128)


@pytest.mark.parametrize("guided", [True, False])
def test_latent_64_is_the_two_argument_call(guided):
    """bench.py calls batch_for_free_hbm(free, guided): the 512 x 512 choice must not move, its floor of 8 included."""
    from distdiff_amd.engine import batch_for_free_hbm
    for free in SWEEP:
        assert batch_for_free_hbm(free, guided, latent_size=64) == batch_for_free_hbm(free, guided), free
    assert batch_for_free_hbm(0, guided, latent_size=64) == 8
    assert batch_for_free_hbm(300 * GB, guided, latent_size=64) == 32


@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("latent", LATENTS)
def test_monotone_in_free_hbm(latent, guided):
    from distdiff_amd.engine import batch_for_free_hbm
    got = [batch_for_free_hbm(free, guided, latent_size=latent) for free in SWEEP]
    assert all(a <= b for a, b in zip(got, got[1:])), (latent, got)
    assert set(got) <= ({8, 16, 32} if latent == 64 else {1, 2, 4, 8, 16, 32})


@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("latent", [48, 96])
def test_chosen_batch_fits_its_prediction(latent, guided):
    """Never a batch whose predicted workspace exceeds the free HBM, unless nothing fits (1)."""
    from distdiff_amd.engine import HBM_BYTES_FIXED, HBM_BYTES_PER_IMAGE_GUIDED, HBM_BYTES_PER_IMAGE_PLAIN, batch_for_free_hbm, predicted_workspace_bytes
    per = (HBM_BYTES_PER_IMAGE_GUIDED if guided else HBM_BYTES_PER_IMAGE_PLAIN) * (latent / 64) ** 2
    for free in SWEEP:
        B = batch_for_free_hbm(free, guided, latent_size=latent)
        assert predicted_workspace_bytes(B, guided, latent) == pytest.approx(B * per + HBM_BYTES_FIXED)
        assert B == 1 or B * per + HBM_BYTES_FIXED <= free, (free, B)
        if B < 32:      # and the next candidate up does not fit
            assert 2 * B * per + HBM_BYTES_FIXED > free, (free, B)


def test_768_pixels_on_an_empty_mi355x():
    """288 GB of HBM: 16 images of 768 x 768 with transform guidance are predicted at 16 x 13.2 + 12 = 223 GB and fit; 32 do not."""
    from distdiff_amd.engine import batch_for_free_hbm
    assert batch_for_free_hbm(280 * GB, True, latent_size=96) == 16
    assert batch_for_free_hbm(200 * GB, True, latent_size=96) == 8
    assert batch_for_free_hbm(280 * GB, True, latent_size=32) == 32


def test_auto_engine_batch_on_cpu_is_unchanged():
    from distdiff_amd.generate_data import auto_engine_batch, parse_args
    assert auto_engine_batch(parse_args(["--synthetic", "4", "--tiny"]), "cpu") == 8
    for res in ("256", "384", "512", "768"):
        assert auto_engine_batch(parse_args(["--synthetic", "4", "--resolution", res]), "cpu") == 16
