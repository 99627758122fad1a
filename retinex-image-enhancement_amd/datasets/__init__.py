from .dataset import (LowLightDataset, LowLightTestDataset, DeviceLoader, draw_params,  # noqa: F401
                      get_train_dataloader, get_test_dataloader)
