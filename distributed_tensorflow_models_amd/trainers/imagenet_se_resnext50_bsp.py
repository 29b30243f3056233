"""Entry script: reference (none: SE-ResNeXt-50 32x4d, models/slim_nets.py resnext with se_ratio=16) (preset ``se_resnext50``, default sync mode ``bsp``).

Accepts the reference flags (--job_name/--ps_hosts/--worker_hosts/--task_id/--batch_size/--data_dir/
--train_dir/--max_steps ...) plus the MI355X extras (--sync_mode, --synthetic_data, --fresh, ...).
"""
from ..compat import flags
from .. import trainer

trainer.define_common_flags(flags, "se_resnext50")


def main(_argv=None):
    return trainer.train("se_resnext50", flags, default_mode="bsp")


if __name__ == "__main__":
    flags.run(main)
