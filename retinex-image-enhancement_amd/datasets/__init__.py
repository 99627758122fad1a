from .dataset import (LowLightDataset, LowLightTestDataset, PairedLowLightDataset, DeviceLoader,  # noqa: F401
                      draw_params, get_train_dataloader, get_test_dataloader)
